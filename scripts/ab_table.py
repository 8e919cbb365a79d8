"""One table from a parent / child / parent / child measurement: every time a throughput script reports, per run, and the verdict.

    python scripts/ab_table.py DIR NAME [NAME ...]        # reads DIR/NAME_{parent,child}{1,2}.json

A figure is a leaf of the result file that is a float, or a list of floats (its median is taken), whose path names a time
(`seconds`, `median`, `*_ms`, `*_s`); counts, rates and ratios derived from them are left out.  The two parent runs give the spread
- the noise floor of the box: nothing tighter can be claimed -, and a child run is `ok` while it is no slower than the slower parent
run plus that spread again.  Prints markdown."""
import json
import os
import statistics
import sys


def figures(x, path=""):
    if isinstance(x, dict):
        for k, v in x.items():
            if k != "box":
                yield from figures(v, f"{path}/{k}")
    elif isinstance(x, list) and x and all(isinstance(v, dict) for v in x):
        for i, v in enumerate(x):
            yield from figures(v, f"{path}[{i}]")
    else:
        leaf = path.rsplit("/", 1)[-1]
        timed = (leaf in ("seconds", "kernel_seconds", "median") or leaf.endswith(("_ms", "_s", "_seconds"))) and "spread" not in leaf
        vals = x if isinstance(x, list) else [x]
        if timed and vals and all(isinstance(v, float) for v in vals):
            yield path, statistics.median(vals)


def main(folder, names):
    print("| figure | parent 1 | parent 2 | child 1 | child 2 | spread | slower parent + spread | verdict |")
    print("|---|---|---|---|---|---|---|---|")
    worst = True
    for name in names:
        runs = {r: dict(figures(json.load(open(os.path.join(folder, f"{name}_{r}.json"))))) for r in ("parent1", "parent2", "child1", "child2")}
        for path in runs["parent1"]:
            if not all(path in r for r in runs.values()):
                continue
            p1, p2, c1, c2 = (runs[r][path] for r in ("parent1", "parent2", "child1", "child2"))
            spread = abs(p1 - p2)
            bound = max(p1, p2) + spread
            ok = max(c1, c2) <= bound
            worst = worst and ok
            print(f"| {name}{path} | {p1:.6g} | {p2:.6g} | {c1:.6g} | {c2:.6g} | {spread:.3g} | {bound:.6g} | {'ok' if ok else 'SLOWER'} |")
    return 0 if worst else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2:]))
