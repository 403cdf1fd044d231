#!/usr/bin/env python3
"""Digest of a ``rocprofv3 --kernel-trace --output-format csv`` run of the plain C3 headline:
where a step's time goes on the GPU, and where the hit ordering of step k runs relative to the scan of step k + 1.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 20 --warmup 3 [--serial-sort]
    python tools/step_trace.py DIR [--steps 20] [--label NAME]

The timed steps are the last ``--steps`` scan dispatches.  All figures are medians over them, in microseconds, from the
dispatches' begin and end timestamps (GPU clock).  A step on the GPU is scan start to scan start; what the scan itself
does not fill is split into
  * waiting for the ordering: the part of [end of scan k, start of the next step's first kernel] before the ordering
    that step k + 1 waits for has ended (two buffers: that of step k - 1; --serial: that of step k, which is then the
    sort itself on the critical path plus the idle time in front of it),
  * other kernels: the counter's zero-fill and the pre-pass of step k + 1,
  * gaps: the rest, i.e. nothing of this process running on the main stream.
The scan's duration in every step of the run (warm-up included) is listed too: the headline's 23 ms of work start on an
idle device, and the trace shows what the clock does to the scan meanwhile.
"""
import argparse
import csv
import glob
import os
import statistics as st
import sys

SCAN, PACK, SORT = "indel_raw_coarse_kernel", "c3c_pack_left_kernel", "small_sort_kernel"


def load(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {path}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                             r.get("LDS_Block_Size", ""), r.get("VGPR_Count", ""), r.get("Workgroup_Size", r.get("Workgroup_Size_X", ""))))
    rows.sort()
    return rows


def med(xs):
    return st.median(xs) / 1000.0 if xs else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--serial", action="store_true", help="the trace of a --serial-sort run")
    a = ap.parse_args()
    rows = load(a.trace)
    scans = [r for r in rows if SCAN in r[2]]
    sorts = [r for r in rows if SORT in r[2]]
    if len(scans) < a.steps + 1:
        raise SystemExit(f"{len(scans)} scan dispatches, need more than {a.steps}")
    first = len(scans) - a.steps
    print(f"# {a.label}: {len(rows)} dispatches, {len(scans)} scans, {len(sorts)} sorts; timed steps = the last {a.steps} scans")
    names = {}
    t_lo, t_hi = scans[first - 1][1], scans[-1][1]
    for r in rows:
        if t_lo <= r[0] <= t_hi + 200000:
            key = (r[2][:90], r[3], r[4], r[5])
            names[key] = names.get(key, 0) + 1
    for (n, lds, vg, wg), c in sorted(names.items(), key=lambda kv: -kv[1]):
        print(f"#   {c:4d} x {n}  (lds {lds}, vgpr {vg}, workgroup {wg})")

    print("# scan us, every step of the run: " + " ".join(str(round((r[1] - r[0]) / 1000.0)) for r in scans))

    def sort_after(t):  # the ordering launched behind the scan that ended at t
        for s in sorts:
            if s[0] >= t:
                return s
        return None

    m = {k: [] for k in ("period", "scan", "end_to_next", "end_to_zero", "zero", "zero_to_pack", "pack", "pack_to_scan",
                         "zero_to_scan", "sort", "sort_delay", "sort_start_vs_next_start", "sort_end_vs_next_end",
                         "sort_end_vs_next_start", "wait", "other", "gaps")}
    serial = 0
    paired = len(sorts) == len(scans)  # one ordering per step: the n-th sort belongs to the n-th scan
    for k in range(first, len(scans) - 1):
        sc, nx = scans[k], scans[k + 1]
        between = [r for r in rows if sc[1] <= r[0] < nx[0] and r is not nx]
        srt = sorts[k] if paired else sort_after(sc[1])
        main_k = [r for r in between if SORT not in r[2]]
        packs = [r for r in main_k if PACK in r[2]]
        zeros = [r for r in main_k if PACK not in r[2]]
        m["period"].append(nx[0] - sc[0])
        m["scan"].append(sc[1] - sc[0])
        m["end_to_next"].append(nx[0] - sc[1])
        head = min((r[0] for r in main_k), default=nx[0])
        if zeros:
            z = zeros[0]
            m["end_to_zero"].append(z[0] - sc[1])
            m["zero"].append(z[1] - z[0])
            m["zero_to_scan"].append(nx[0] - z[0])
            if packs:
                m["zero_to_pack"].append(packs[0][0] - z[1])
        if packs:
            m["pack"].append(packs[0][1] - packs[0][0])
            m["pack_to_scan"].append(nx[0] - packs[0][1])
        other = sum(r[1] - r[0] for r in main_k)
        wait = 0
        if srt is not None:
            m["sort"].append(srt[1] - srt[0])
            m["sort_delay"].append(srt[0] - sc[1])
            m["sort_start_vs_next_start"].append(srt[0] - nx[0])
            m["sort_end_vs_next_end"].append(srt[1] - nx[1])
            m["sort_end_vs_next_start"].append(srt[1] - nx[0])
            if srt[1] <= nx[0]:  # the sort ran between the two scans: on the critical path
                serial += 1
        # the ordering the next step's buffer waits for: that of step k - 1 (two buffers), serial: that of step k
        awaited = srt if a.serial else (sorts[k - 1] if paired and k >= 1 else None)
        if awaited is not None:
            wait = max(0, min(awaited[1], head) - sc[1])
        m["wait"].append(wait)
        m["other"].append(other)
        m["gaps"].append((nx[0] - sc[1]) - wait - other)
    print(f"step on the GPU (scan start to scan start)        {med(m['period']):9.1f} us")
    print(f"scan                                               {med(m['scan']):9.1f} us")
    print(f"end of scan k -> start of scan k+1                 {med(m['end_to_next']):9.1f} us")
    print(f"  end of scan k -> start of zero-fill k+1          {med(m['end_to_zero']):9.1f} us")
    print(f"  zero-fill                                        {med(m['zero']):9.1f} us")
    print(f"  zero-fill end -> pre-pass start                  {med(m['zero_to_pack']):9.1f} us")
    print(f"  pre-pass                                         {med(m['pack']):9.1f} us")
    print(f"  pre-pass end -> scan start                       {med(m['pack_to_scan']):9.1f} us")
    print(f"  zero-fill start -> scan start                    {med(m['zero_to_scan']):9.1f} us")
    print(f"small_sort_kernel of step k: duration              {med(m['sort']):9.1f} us")
    print(f"  start - end of scan k                            {med(m['sort_delay']):+9.1f} us")
    print(f"  start - start of scan k+1                        {med(m['sort_start_vs_next_start']):+9.1f} us")
    print(f"  end   - start of scan k+1                        {med(m['sort_end_vs_next_start']):+9.1f} us")
    print(f"  end   - end of scan k+1                          {med(m['sort_end_vs_next_end']):+9.1f} us")
    print(f"  sorts that ended before scan k+1 began           {serial:5d} of {len(m['sort'])}")
    print(f"split of step - scan = {med(m['end_to_next']):.1f} us: waiting for the ordering {med(m['wait']):.1f}, other kernels "
          f"{med(m['other']):.1f}, gaps {med(m['gaps']):.1f}")


if __name__ == "__main__":
    sys.exit(main())
