#!/usr/bin/env python3
"""What could a guessed starting threshold gain the screened top-k at most?

The screen kernel's survivor handling depends on the bound a row carries while
the corpus streams past.  The best bound any guess could give a row from the
first tile on is the one the row ends the pass with.  This experiment measures
that ceiling on the benchmark's config (c3 unless --config says otherwise):

  1. one step as shipped, saving gthr (the rows' proven bounds) after the
     screen kernel;
  2. steps whose rows start from the saved bounds instead of the seed's.  The
     saved bounds are proven, so the results are those of the shipped path.

Needs the experiment build of the library:

  make -C polars-matmul_amd ab AB=-DPMM_SCREEN_CEILING AB_NAME=libpmm_ceiling.so

Runs bench.py (a fresh process each time) normal / preloaded alternated
--pairs times and prints, per run, the step, `gemm_f32_topk/screen` per launch
and the screen's debug counters; with --out DIR the bench lines are kept there.
The preloaded step's wall time includes reading and uploading the bounds, so
compare the kernel times.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench(env_extra, config, steps, warmup, timeout):
    env = dict(os.environ, PMM_LIB="libpmm_ceiling.so", PMM_SCREEN_DEBUG="1")
    env.pop("PMM_SCREEN_GTHR_LOAD", None)
    env.pop("PMM_SCREEN_GTHR_SAVE", None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", str(steps),
                        "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"bench.py exited with {p.returncode}")
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    dbg = [ln for ln in p.stderr.splitlines() if ln.startswith("[pmm screen]")]
    counters = dict(re.findall(r"(\w+)=(\S+)", dbg[-1])) if dbg else {}
    return line, counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per bench.py run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        saved = os.path.join(tmp, "gthr.bin")
        bench({"PMM_SCREEN_GTHR_SAVE": saved}, args.config, 1, 0, args.timeout)
        print(f"saved {os.path.getsize(saved) // 8} bounds", flush=True)
        rows = []
        for i in range(args.pairs):
            for kind, extra in (("normal", {}), ("preloaded", {"PMM_SCREEN_GTHR_LOAD": saved})):
                line, c = bench(extra, args.config, args.steps, args.warmup, args.timeout)
                roof = line.get("roofline") or {}
                row = {"run": i + 1, "kind": kind, "ms_per_step": line.get("ms_per_step"),
                       "screen_ms": roof.get("kernel_ms_avg"), "merge_ms_avg": roof.get("merge_ms_avg"),
                       "rescored": c.get("rescored"), "max_per_row": c.get("max_per_row"),
                       "rerun_rows": c.get("rerun_rows"), "overflowed": c.get("overflowed")}
                rows.append(row)
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(os.path.join(args.out, f"{args.config}_{kind}_{i + 1}.json"), "w") as f:
                        f.write(json.dumps(line) + "\n")
    for kind in ("normal", "preloaded"):
        v = sorted(r["screen_ms"] for r in rows if r["kind"] == kind and r["screen_ms"] is not None)
        if v:
            print(f"{kind}: screen kernel ms per launch min {v[0]} median {v[len(v) // 2]} max {v[-1]}")


if __name__ == "__main__":
    main()
