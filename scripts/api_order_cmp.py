"""Same calls in the same order? (measurement only)  Three `scripts/api_trace.py DIR --lists` outputs
of scripts/block_commit_prof.py -- a base build traced twice, then the build under test -- compared
per timed block and host thread: the ordered HIP function names and the ordered names of the kernels
the thread launched.  Where the base differs from itself (the account phase polls hipEventQuery),
the calls whose counts vary are named, their counts given for all three runs, and the order is
compared with those calls taken out.

  python scripts/api_order_cmp.py base1.json base2.json new.json > profiles/<tag>_api_trace.json
"""
import collections
import json
import sys


def main():
    P1, P2, N = (json.load(open(f)) for f in sys.argv[1:4])
    out = {"workload": "scripts/block_commit_prof.py under rocprofv3 --hip-trace --kernel-trace, "
                       "scripts/api_trace.py --lists; threads in the order of their first call in the block",
           "blocks": []}
    ok = len(P1) == len(P2) == len(N)
    for b, (p1, p2, n) in enumerate(zip(P1, P2, N)):
        rb = {"block": b, "kernels_base_base_new": [p1["kernels"], p2["kernels"], n["kernels"]],
              "host_threads_base_base_new": [len(x["threads"]) for x in (p1, p2, n)], "threads": []}
        ok &= len(set(rb["host_threads_base_base_new"])) == 1
        for t, (a1, a2, an) in enumerate(zip(p1["threads"].values(), p2["threads"].values(), n["threads"].values())):
            rt = {"thread": t, "calls_base_base_new": [len(x["functions"]) for x in (a1, a2, an)]}
            for what in ("functions", "kernels"):
                c1, c2, cn = (collections.Counter(x[what]) for x in (a1, a2, an))
                vary = sorted(k for k in set(c1) | set(c2) if c1[k] != c2[k])
                l1, l2, ln = ([x for x in a[what] if x not in vary] for a in (a1, a2, an))
                r = {"base_equals_itself": a1[what] == a2[what]}
                if l1 == l2:  # the base agrees with itself on everything but the calls that vary
                    r.update(compared="order" + (" without the calls whose count varies in the base; those by count"
                                                 if vary else ""),
                             calls_compared_in_order=len(l1), new_equals_base=l1 == ln)
                else:  # the base's own two orders differ: counts only
                    r.update(compared="counts per name (the base's two runs order the same calls differently)",
                             new_equals_base=all(cn[k] == c1[k] for k in set(c1) | set(cn) if k not in vary))
                if vary:
                    r["counts_that_vary_base_base_new"] = {k: [c1[k], c2[k], cn[k]] for k in vary}
                if not r["new_equals_base"] and l1 == l2:
                    k = next((i for i, (x, y) in enumerate(zip(l1, ln)) if x != y), min(len(l1), len(ln)))
                    r["first_difference"] = [k, l1[k:k + 4], ln[k:k + 4]]
                ok &= r["new_equals_base"]
                rt[what] = r
            rb["threads"].append(rt)
        out["blocks"].append(rb)
    out["same_calls_in_the_same_order"] = bool(ok)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
