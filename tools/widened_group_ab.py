"""Fold the lines of tools/widened_group_ab.cpp's runs into profiles/widened_group_ab.json.

    python tools/widened_group_ab.py --a A1 A2 A3 --b B1 B2 B3 --off O1 O2 O3 > profiles/widened_group_ab.json

Each argument is the stdout of one process: arm A (this tree's library), arm B (the library of the commit before
widened runs were coalesced), and arm A under DCCL_GROUP_COALESCE=0.  Per case the profile keeps every process's
median [min, max] us per group, the median of the processes' medians with the extremes over all of them, B / A, and
whether all runs of all arms gave one output hash.
"""
import argparse
import json
import statistics
import sys


def load(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            runs.append([json.loads(l) for l in f if l.startswith("{")])
    return runs


def fold(runs, key):
    rows = [r for run in runs for r in run if r["case"] == "group" and (r["payload_bytes"], r["accumulate"]) == key]
    return {"us": statistics.median(r["us"] for r in rows), "us_min": min(r["us_min"] for r in rows),
            "us_max": max(r["us_max"] for r in rows), "processes": [[r["us"], r["us_min"], r["us_max"]] for r in rows],
            "hashes": sorted({r["hash"] for r in rows})}


def main():
    ap = argparse.ArgumentParser()
    for arm in ("a", "b", "off"):
        ap.add_argument(f"--{arm}", nargs="+", required=True)
    args = ap.parse_args()
    arms = {arm: load(getattr(args, arm)) for arm in ("a", "b", "off")}
    keys = sorted({(r["payload_bytes"], r["accumulate"]) for r in arms["a"][0] if r["case"] == "group"})
    out = {"shape": "W = 4 thread ranks, one MI355X, direct path, bf16, 16 same-handle widened reduce-scatters per "
                    "group; us per group of the slowest rank, median [min, max]; DCCL_GROUP_COALESCE_MAX_BYTES = 1 GiB",
           "cases": [], "kernel": [r for run in arms["a"] for r in run if r["case"] == "kernel"]}
    for key in keys:
        a, b, off = (fold(arms[arm], key) for arm in ("a", "b", "off"))
        out["cases"].append({"payload_bytes": key[0], "accumulate": key[1], "a": a, "b": b, "a_coalesce_off": off,
                             "b_over_a": round(b["us"] / a["us"], 3),
                             "b_over_a_worst": round(b["us_min"] / a["us_max"], 3),
                             "off_inside_b_band": b["us_min"] <= off["us"] <= b["us_max"],
                             "hashes_agree": len(set(a["hashes"] + b["hashes"] + off["hashes"])) == 1})
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
