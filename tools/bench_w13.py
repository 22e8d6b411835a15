#!/usr/bin/env python
"""13-bit weight planes (csrc/w13.h) against the bf16 rows, kernel by kernel: every role of a bf16 context alone, back to back over all
layers' weights between one pair of HIP events (dtk_bench_gemv), the bf16 kernel the step would run (0x2000 | 0xff), what the step
streams (0xff) and every 13-bit shape (0x1000 | shape) alternating in one process; us per launch.  Each shape runs twice a round: with
the rows' zero-code flags as packed (rows without a zero code take the short decode) and, "_general", with every row flagged (option
w13_nz = 0: the general decode everywhere).  Also the rows flagged per role and the cost of packing (the first call packs every matrix:
wall time around it).  Writes profiles/w13_<model>_chains.json, which profiles/w13_<model>.json quotes.

    python tools/bench_w13.py [--model detikzify-ds-7b] [--rounds 3] [--chain-reps 8]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ROLES = ["qkv", "o_proj", "gate_up", "down", "lm_head"]
# the shapes that fold the RMSNorm sum of squares as 4 waves do in a block of 8 / 16 (k_gemv's FW): persistent, blocks per CU 2 / 1
NAMES = {0: {6: "persistent R1 U4 8 waves, fold 4", 7: "persistent R1 U4 16 waves, fold 4"},
         2: {6: "persistent R1 U4 8 waves, fold 4", 7: "persistent R1 U4 16 waves, fold 4"},
         4: {5: "persistent R2 U4 8 waves, fold 4", 6: "persistent R1 U4 8 waves, fold 4", 7: "persistent R2 U4 16 waves, fold 4"}}
SHAPES = {0: range(8), 1: range(7), 2: range(8), 3: range(7), 4: range(8)}      # (o_proj, through PRO_COPY: the step keeps its bf16 rows, dtk_bench_gemv packs it for the call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain-reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import detikzify_amd.model as dmodel
    m, _ = dmodel.load(args.model, synthetic=1234)
    m.set_option("w13", 1)
    import time
    t0 = time.perf_counter()
    us = C.c_float(0.0)
    m._check(m.lib.dtk_bench_gemv(m._ctx, 2, 0xFF, 1, C.byref(us)), "dtk_bench_gemv")      # packs (ensure_w13) + 2 passes of gate/up
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    m._check(m.lib.dtk_bench_gemv(m._ctx, 2, 0xFF, 1, C.byref(us)), "dtk_bench_gemv")
    pack_ms = round((first - (time.perf_counter() - t0)) * 1e3, 1)

    def chain(role, variant):
        us = C.c_float(0.0)
        m._check(m.lib.dtk_bench_gemv(m._ctx, role, variant, args.chain_reps, C.byref(us)), "dtk_bench_gemv")
        return round(float(us.value), 3)

    flagged = {r: int(m.lib.dtk_w13_flagged_rows(m._ctx, i)) for i, r in enumerate(ROLES)}
    res = {r: {"bf16": []} for r in ROLES}
    for _ in range(args.rounds):
        for nz in (1, 0):
            m.set_option("w13_nz", nz)              # (packs again: every row byte is rewritten)
            tag = "" if nz else "_general"
            for i, r in enumerate(ROLES):
                res[r]["bf16"].append(chain(i, 0xFF | 0x2000))
                res[r].setdefault("step" + tag, []).append(chain(i, 0xFF))
                for v in SHAPES[i]:
                    res[r].setdefault(f"w13_shape_{v}{tag}", []).append(chain(i, 0x1000 | v))
                res[r]["bf16"].append(chain(i, 0xFF | 0x2000))
    m.set_option("w13_nz", 1)
    st = m.stats()
    out = {"model": args.model, "measured": "us per launch, chains over all layers' weights, one process",
           "w13_counts": {"packed": st["w13_counts"] & 1023, "unpacked": (st["w13_counts"] >> 10) & 1023, "unpackable_rows": st["w13_counts"] >> 20},
           "weight_bytes_per_token": int(st["weight_bytes_per_token"]), "probe_kernel_bytes": int(st["probe_kernel_bytes"]),
           "pack_all_matrices_ms": pack_ms, "rows_with_a_zero_code": flagged, "fold_4_shapes": {ROLES[i]: n for i, n in NAMES.items()},
           "chains": res, "median_us": {r: {k: statistics.median(v) for k, v in d.items()} for r, d in res.items()}}
    path = Path(args.out) if args.out else ROOT / "profiles" / f"w13_{args.model.replace('detikzify-', '')}_chains.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["median_us"], indent=1))


if __name__ == "__main__":
    main()
