"""Dev tool: what the render MLP's launches (`k_field<L, false, 0, 4, true>`, the planes route behind `k_encode_xcd`) do inside
a rocprofv3 kernel trace of a bench run: per launch the duration, the gap between the end of the preceding `k_encode_xcd` of
the same stream and its start, and which kernels of OTHER streams run during it (share of the launch's interval they cover).
Compare a three-in-flight trace with a `--in-flight 1` trace: launches that are longer or later with three frames in flight are
the ones that wait for CUs.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python bench.py --steps 200 --warmup 20 [--in-flight 1]
    python tools/field_coresidency.py DIR/.../r_kernel_trace.csv [frames]      (the last `frames` frames, default 150)

Another kernel is looked at the same way with `--kernel NAME [--after PREDECESSOR]`: every launch whose name contains NAME, the gap
behind the last launch of the same stream whose name contains PREDECESSOR.  The hash-grid encoder behind its stream's search:
    python tools/field_coresidency.py DIR/.../r_kernel_trace.csv [frames] --kernel k_encode_xcd --after k_search
"""
import bisect
import collections
import csv
import re
import statistics
import sys

FIELD = re.compile(r"k_field<\s*(8|16),\s*false,\s*0,\s*4,\s*true\s*>")


def short(name):
    m = re.search(r"(k_\w+)", name)
    return m.group(1) if m else name.split("(")[0][-40:]


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def main(path, frames=150, kernel=None, after="k_encode_xcd"):
    match = (lambda n: kernel in n) if kernel else FIELD.search
    label = kernel if kernel else "k_field<L,false,0,4,true>"
    rows = list(csv.DictReader(open(path)))
    key = "Stream_Id" if rows and "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows}) > 1 else "Queue_Id"
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r[key],
           int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0),
           r.get("VGPR_Count", "?"), r.get("LDS_Block_Size", "?")) for r in rows]
    ks.sort()
    probes = [k[0] for k in ks if "k_probe_points" in k[2]]
    t0 = probes[-frames] if len(probes) >= frames else (probes[0] if probes else ks[0][0])
    ks = [k for k in ks if k[0] >= t0]
    n_frames = sum(1 for k in ks if "k_probe_points" in k[2])
    span = (max(k[1] for k in ks) - ks[0][0]) / 1e3
    print("trace %s: %d launches, %d frames analysed (%.1f us per frame), streams keyed by %s (%d distinct)"
          % (path.split("/")[-1], len(ks), n_frames, span / max(n_frames, 1), key, len({k[3] for k in ks})))
    starts = [k[0] for k in ks]
    longest = max(k[1] - k[0] for k in ks)
    last_enc = {}
    dur, gap, cover = [], [], collections.defaultdict(float)
    search_cov, alone, shape = [], 0, collections.Counter()
    for i, (s, e, name, q, wg, grid, vgpr, lds) in enumerate(ks):
        if not match(name):
            if after in name:
                last_enc[q] = e
            continue
        shape[(wg, vgpr, lds)] += 1
        dur.append((e - s) / 1e3)
        if q in last_enc:
            gap.append((s - last_enc[q]) / 1e3)
        ov = collections.defaultdict(float)
        for j in range(bisect.bisect_left(starts, s - longest), bisect.bisect_left(starts, e)):
            s2, e2, n2, q2 = ks[j][:4]
            if j != i and q2 != q and e2 > s and s2 < e:
                ov[short(n2)] += (min(e, e2) - max(s, s2)) / max(e - s, 1)
        for k, v in ov.items():
            cover[k] += v
        search_cov.append(min(ov.get("k_search", 0.0), 3.0))
        alone += not ov
    n = len(dur)
    if not n:
        print("no %s launch found" % (kernel or "k_field<L, false, 0, 4, true>"))
        return
    print("%s: %d launches (%.1f per frame); (threads per workgroup, VGPRs, LDS bytes): %s"
          % (label, n, n / max(n_frames, 1), sorted(shape.items())))
    print("  duration us   mean %.1f  median %.1f  p90 %.1f  max %.1f   sum per frame %.1f us"
          % (statistics.mean(dur), statistics.median(dur), pct(dur, 0.9), max(dur), sum(dur) / max(n_frames, 1)))
    if gap:
        print("  gap after the stream's %s us   mean %.1f  median %.1f  p90 %.1f  max %.1f   sum per frame %.1f us"
              % (after, statistics.mean(gap), statistics.median(gap), pct(gap, 0.9), max(gap), sum(gap) / max(n_frames, 1)))
    print("  launches with no kernel of another stream running during them: %d (%.0f %%)" % (alone, 100.0 * alone / n))
    print("  k_search launches of other streams running during a launch (time-weighted mean count): %.2f" % statistics.mean(search_cov))
    print("  kernels of other streams during a launch, mean share of its interval covered (can exceed 1: several streams):")
    for k, v in sorted(cover.items(), key=lambda kv: -kv[1])[:8]:
        print("    %-28s %.2f" % (k, v / n))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("frames", nargs="?", type=int, default=150)
    ap.add_argument("--kernel", default=None, help="substring of the kernel's name (default: the planes-route render MLP)")
    ap.add_argument("--after", default="k_encode_xcd", help="substring of the same stream's predecessor, for the gap line")
    a = ap.parse_args()
    main(a.trace, a.frames, a.kernel, a.after)
