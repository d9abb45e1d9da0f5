#!/usr/bin/env python3
"""Executed vector instructions per NARROW and per WIDE wavefront of the raw-byte decimator (k_pz_raw), from two counter
passes at chunk lengths with different block counts.

A row of n samples is nb = ceil((P0 + n + 54) / (64 L)) blocks of one wavefront each; block 0 and the blocks from
b_tail = min((P0 + 27 + n) // (64 L), nb - 1) on run the wide body, the others the narrow one (ref_pipeline.hpp run_pz_raw,
tests/raw_matrix.geometry).  SQ_INSTS_VALU / SQ_WAVES of a launch is the average over its wavefronts, so per pass
    nb * average = narrow * V_narrow + wide * V_wide,
and two passes whose narrow : wide ratios differ give both unknowns.  At q = 10 (L = 120) chunks of 262 144 and 131 072
samples are 33 + 2 and 16 + 2 blocks.

The two-equation solution takes a wide wavefront to execute the same count at both lengths.  That holds for the
cooperative edge fill (fully unrolled, the same for every row end), not for the per-lane rolled loop it replaced
(tdm_debug_set "raw_edge_fill" 0, and every build before the fill): an iteration of that loop is longer for a sample of the
row than for a pad position, so its count moves with where the signal ends inside its lane (64 samples into the lane at
262 144, 32 at 131 072: about 200 instructions per wide wavefront), and the difference lands in V_narrow.  --narrow V takes
the narrow count as known, e.g. from a build with the fill whose narrow body is the same, and gives V_wide per pass.

Each pass is a directory written by
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES [...] --kernel-trace --output-format csv -d DIR -- python bench.py --depth 1 --chunk N ...
(as tools/pmc_sq.sh runs its passes: counters alone, nothing else traced).

usage: tools/raw_block_kinds.py DIR_A CHUNK_A DIR_B CHUNK_B [--lane L] [--narrow V] [--json OUT]   (default L = 120: q = 10, S = 12)
"""
import argparse
import collections
import csv
import glob
import json
import os

EDGE = 27


def geometry(L, n):
    B = 64 * L
    P0 = (L - EDGE % L) % L
    nb = (P0 + n + 2 * EDGE + B - 1) // B
    b_tail = min((P0 + EDGE + n) // B, nb - 1)
    wide = (nb - b_tail) + (1 if b_tail > 0 else 0)
    return nb, nb - wide, wide


def per_wave(directory, kernel="k_pz_raw"):
    """(average SQ_INSTS_VALU per wavefront over the kernel's launches, launches)"""
    files = glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit(f"{directory}: no *counter_collection.csv")
    acc = collections.defaultdict(dict)
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if kernel in r["Kernel_Name"] and r["Counter_Name"] in ("SQ_INSTS_VALU", "SQ_WAVES"):
                    d = acc[(f, r.get("Dispatch_Id") or r.get("Correlation_Id"))]   # (a counter may come in several rows: summed)
                    d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    ratios = [d["SQ_INSTS_VALU"] / d["SQ_WAVES"] for d in acc.values() if d.get("SQ_WAVES") and "SQ_INSTS_VALU" in d]
    if not ratios:
        raise SystemExit(f"{directory}: no launch of {kernel} with SQ_INSTS_VALU and SQ_WAVES")
    return sum(ratios) / len(ratios), len(ratios)


def solve(avg_a, geo_a, avg_b, geo_b):
    """geo = (nb, narrow, wide) -> (V_narrow, V_wide)"""
    (nba, na, wa), (nbb, nbn, wb) = geo_a, geo_b
    det = na * wb - nbn * wa
    if det == 0:
        raise SystemExit("the two chunk lengths have the same narrow : wide ratio; take lengths with different block counts")
    ta, tb = nba * avg_a, nbb * avg_b
    return (ta * wb - tb * wa) / det, (na * tb - nbn * ta) / det


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir_a")
    ap.add_argument("chunk_a", type=int)
    ap.add_argument("dir_b")
    ap.add_argument("chunk_b", type=int)
    ap.add_argument("--lane", type=int, default=120, help="samples per lane, Q * S")
    ap.add_argument("--narrow", type=float, default=None, help="known vector instructions per narrow wavefront: V_wide per pass")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    a = ap.parse_args()
    geo_a, geo_b = geometry(a.lane, a.chunk_a), geometry(a.lane, a.chunk_b)
    avg_a, la = per_wave(a.dir_a)
    avg_b, lb = per_wave(a.dir_b)
    vn, vw = solve(avg_a, geo_a, avg_b, geo_b)
    out = {"lane": a.lane,
           "passes": [{"chunk": a.chunk_a, "blocks": geo_a[0], "narrow": geo_a[1], "wide": geo_a[2], "launches": la, "valu_per_wave": avg_a},
                      {"chunk": a.chunk_b, "blocks": geo_b[0], "narrow": geo_b[1], "wide": geo_b[2], "launches": lb, "valu_per_wave": avg_b}],
           "valu_per_narrow_wave": vn, "valu_per_wide_wave": vw}
    for p in out["passes"]:
        print(f"chunk {p['chunk']}: {p['blocks']} blocks = {p['narrow']} narrow + {p['wide']} wide, {p['launches']} launches, "
              f"SQ_INSTS_VALU / SQ_WAVES = {p['valu_per_wave']:.1f}")
    print(f"vector instructions per narrow wavefront {vn:.0f}, per wide wavefront {vw:.0f}")
    if a.narrow is not None:
        out["given_narrow"] = a.narrow
        for p in out["passes"]:
            p["valu_per_wide_wave_given_narrow"] = (p["blocks"] * p["valu_per_wave"] - p["narrow"] * a.narrow) / p["wide"]
            print(f"with {a.narrow:.0f} per narrow wavefront: chunk {p['chunk']}: {p['valu_per_wide_wave_given_narrow']:.0f} per wide wavefront")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
