"""Generates tests/golden/fx_walk_census.json: the grid walks' census (tests/walk_census.py) of the library as built -- the integer read-outs `candidates`
and `grown` of the search index, the outlier filters and Euclidean clustering, rgc_gicpmp_num_candidates and a SHA-256 of FastGICPMultiPoints' merged()
bytes, for every designed case at the cell sizes the GPU tests use.  Runs the product only (needs the MI355X); record it from the library a change to the
walks is compared against, BEFORE the change.

    python tests/golden/gen_walk_census.py [--out tests/golden/fx_walk_census.json]     # RGC_HIP_LIB=<another build> records that build
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fx_walk_census.json"))
    a = ap.parse_args()
    import walk_census
    rec = walk_census.census()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries -> %s" % (len(rec), a.out))


if __name__ == "__main__":
    main()
