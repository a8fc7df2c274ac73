#!/usr/bin/env python3
"""Summarises SC_LEVEL_LOG files (one per worker slot): per level, time inside the kernel, time between the
request and the observed stamp, host time between levels; for the sampler levels the tail behind the chain (chain's
end -> end of the count over the draw log -> stamp), split by the workgroup that counts (NB = ceil(S / 16) <= 2: eight
wavefronts, NB >= 3: four); for the levels without a sampler how many are hard updates, how many of those carry
duplicates or multi-symbol labels, and their time behind the update.  usage: level_log_summary.py PREFIX"""
import glob
import sys


def rows(prefix):
    for fn in glob.glob(prefix + ".*"):
        for l in open(fn):
            f = l.split()
            if not f or f[0] != "h":
                continue
            d = {}
            i = 0
            try:
                while i < len(f):
                    if f[i] == "ph":
                        # five ticks, or six once the end of the count is stamped too
                        ph = []
                        i += 1
                        while i < len(f) and f[i][0] in "-0123456789.":
                            ph.append(float(f[i]))
                            i += 1
                        d["ph"] = ph
                    else:
                        d[f[i]] = float(f[i + 1])
                        i += 2
            except (ValueError, IndexError):
                continue
            yield d


def avg(xs):
    xs = list(xs)
    return sum(xs) / max(len(xs), 1)


def main():
    rs = list(rows(sys.argv[1]))
    warm = max(r["h"] for r in rs) // 2
    rs = [r for r in rs if r["h"] > warm] or rs
    ch = [r for r in rs if r["chain_us"] > 0]
    pl = [r for r in rs if r["chain_us"] == 0]
    for name, g in (("sampler", ch), ("plain", pl)):
        print("%-8s n %6d  kernel %.1f us (chain %.1f: stage %.1f copies %.1f update %.1f slots %.1f table %.1f)  request->stamp seen %.1f"
              "  (outside kernel %.1f; request->launched %.1f, batch %.1f)  host between levels %.1f" % (
                  name, len(g), avg(r["level_us"] for r in g), avg(r["chain_us"] for r in g), avg(r["ph"][0] for r in g),
                  avg(r["ph"][1] - r["ph"][0] for r in g), avg(r["ph"][2] - r["ph"][1] for r in g), avg(r["ph"][3] - r["ph"][2] for r in g),
                  avg(r["ph"][4] - r["ph"][3] for r in g), avg(r["wait_us"] for r in g), avg(r["wait_us"] - r["level_us"] for r in g),
                  avg(r.get("pend_us", 0) for r in g), avg(r.get("batch", 0) for r in g), avg(r["host_us"] for r in g)))
    # the tail of a sampler level: the chain starts at ph[4] and runs for chain_us
    for name, g in (("all", ch), ("NB<=2", [r for r in ch if r["S"] <= 32]), ("NB>=3", [r for r in ch if r["S"] > 32])):
        if not g:
            continue
        line = "tail %-6s n %6d  S %.1f Q %.1f n_sweeps %.1f  chain's end -> stamp %.2f" % (
            name, len(g), avg(r["S"] for r in g), avg(r["Q"] for r in g), avg(r["n"] for r in g),
            avg(r["level_us"] - r["ph"][4] - r["chain_us"] for r in g))
        if all(len(r["ph"]) > 5 for r in g):
            line += "  (chain's end -> count's end %.2f, count's end -> stamp %.2f)" % (
                avg(r["ph"][5] - r["ph"][4] - r["chain_us"] for r in g), avg(r["level_us"] - r["ph"][5] for r in g))
        print(line)
    # levels without a sampler: mode 0 is the hard update
    hard = [r for r in pl if r["mode"] == 0]
    stay = [r for r in hard if r.get("multi", 0) or r.get("dups", 0)]
    free = [r for r in hard if not (r.get("multi", 0) or r.get("dups", 0))]
    print("plain    n %6d  hard %d, of those with duplicates or multi-symbol labels %d%s" % (
        len(pl), len(hard), len(stay), "" if any("dups" in r for r in pl) else " (multi only: no dups column in this log)"))
    for name, g in (("hard, single symbols, no duplicates", free), ("hard, duplicates or multi", stay)):
        if g:
            print("  %-36s n %6d  S %.1f Q %.1f  level %.1f us, update's end (ph 2) %.1f, ph 2 -> level's end %.1f, on the grid (done & 8) %d" % (
                name, len(g), avg(r["S"] for r in g), avg(r["Q"] for r in g), avg(r["level_us"] for r in g), avg(r["ph"][2] for r in g),
                avg(r["level_us"] - r["ph"][2] for r in g), sum(1 for r in g if int(r.get("done", 0)) & 8)))


if __name__ == "__main__":
    main()
