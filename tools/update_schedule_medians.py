"""median schedule of a graph update over ALL updates of a rocprofv3 kernel trace (one sample says little):
python tools/update_schedule_medians.py <dir with *kernel_trace.csv> -> per (kernel, grid, occurrence): median start, median duration, queue"""
import csv, glob, statistics as st, sys
rows = list(csv.DictReader(open(glob.glob(sys.argv[1] + "/*/*kernel_trace.csv")[0])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
def short(n):
    return n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:44]
starts = [i for i, r in enumerate(rows[:-4]) if "reproject_motion_kernel" in r["Kernel_Name"]
          and any("corr_lookup" in rows[i + k]["Kernel_Name"] for k in (1, 2, 3))]
starts = starts[len(starts) // 3:]                     # the timed steps, not the priming
for want_ctx in (True, False):
    acc, lens = {}, []
    for a, b in zip(starts[:-1], starts[1:]):
        t0 = int(rows[a]["Start_Timestamp"])
        span = (int(rows[b]["Start_Timestamp"]) - t0) / 1e3
        names = [rows[i]["Kernel_Name"] for i in range(a, b)]
        has_ctx = any("gru_glo" in n for n in names)
        if span > 800 or has_ctx != want_ctx:             # (the last update of a step runs into the keyframe boundary)
            continue
        lens.append(span)
        seen = {}
        for i in range(a, b):
            r = rows[i]
            k0 = (short(r["Kernel_Name"]), r.get("Grid_Size_X", r.get("Grid_Size", "?")))
            seen[k0] = seen.get(k0, 0) + 1
            e = acc.setdefault(k0 + (seen[k0],), ([], [], set()))
            e[0].append((int(r["Start_Timestamp"]) - t0) / 1e3); e[1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            e[2].add(r.get("Queue_Id", "?"))
    if not lens:
        continue
    print("updates %s their own gate context: %d, start to next start median %.1f us (min %.1f, max %.1f)" %
          ("WITH" if want_ctx else "without", len(lens), st.median(lens), min(lens), max(lens)))
    for k, (s, d, q) in sorted(acc.items(), key=lambda kv: st.median(kv[1][0])):
        if len(s) >= len(lens) // 2:
            print("%9.1f %8.1f  end %7.1f  q%-4s %s [%s] #%d" % (st.median(s), st.median(d), st.median([x + y for x, y in zip(s, d)]), ",".join(sorted(q)), k[0], k[1], k[2]))
    print()
