"""Join two tools/rocpd_stats.py tables of the same workload — one taken one forward at a time (--streams 1), one under
load (the headline's 32 forwards in flight) — into one markdown table per kernel: mean duration one at a time, mean
duration under load, workgroups x threads x LDS, and the kernel's share of the loaded GPU-busy time.
usage: python tools/loaded_vs_single.py <single.txt> <loaded.txt> [min_calls]"""
import sys


def load(path):
    out = {}
    for line in open(path):
        if line.startswith("#") or line.startswith("kernel "):
            continue
        f = line.rstrip().rsplit(None, 11)
        if len(f) != 12:
            continue
        name, calls, total, avg, _mn, _mx, pct, gx, gy, _vg, lds, wg = f
        out[(name, int(gx), int(gy))] = dict(calls=int(calls), total=float(total), avg=float(avg), pct=float(pct),
                                             wgs=int(gx) * max(int(gy), 1) // max(int(wg), 1), wg=int(wg), lds=int(lds))
    return out


def main(single, loaded, min_calls=500):
    s, l = load(single), load(loaded)
    print("| kernel | one at a time µs | under load µs | workgroups × threads × LDS | loaded GPU-busy % |")
    print("|---|---:|---:|---|---:|")
    for key, v in sorted(l.items(), key=lambda kv: -kv[1]["total"]):
        if v["calls"] < min_calls:          # set-up kernels (weight folding, fills): not part of a forward
            continue
        one = s.get(key)
        print("| `%s` | %s | %.2f | %d × %d × %.1f KB | %.1f |" % (key[0][:60], "%.2f" % one["avg"] if one else "—", v["avg"],
                                                                 v["wgs"], v["wg"], v["lds"] / 1024.0, v["pct"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 500)
