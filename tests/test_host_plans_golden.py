"""The host layer's pure planners against recorded numbers (no GPU).

pmm_shard_plan (the sharded search's memory plan: shard -> plan, plan devices,
plan bytes, list offsets) and pmm_topk_i8_workspace_bytes are integer planning,
so the check is equality.  The library plans for 256 CUs before any probe, and
an MI355X has 256.  tests/golden/shard_plan.json and workspace_i8.json were
recorded from the build before the two sharded planners and the two chunk
schedules became one each; `python tests/test_host_plans_golden.py` records them
again from the library in the tree.  (pmm_topk_workspace_bytes is pinned by the
table in test_workspace_routes.py.)
"""
from __future__ import annotations

import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHARD_PLAN = os.path.join(HERE, "golden", "shard_plan.json")
WORKSPACE_I8 = os.path.join(HERE, "golden", "workspace_i8.json")

DEVICE_LISTS = ([0], [0, 0, 1], [3, 1, 3, 2], [0] * 8)
# (m, n, d, k): the plan tests' shape, shards shorter than k under 8 shards, one
# shard shorter than k beside one that is not, bf16 past d = 768 (widened), a
# d no multiple of the row padding, k at the fused limit
SHAPES = ((1000, 100_003, 768, 100), (37, 100, 40, 64), (33, 129, 40, 65), (256, 16384, 1024, 100),
          (70, 3001, 100, 10), (64, 4099, 256, 1024))

# test_int8_cpu.py's grid (native, several passes, widened past either limit) and small odd shapes
I8_GRID = [(70, 3001, d, k) for d, k in ((1, 1), (768, 100), (1536, 1000), (2048, 1024), (1985, 1024), (2049, 10),
                                         (4096, 10), (64, 1025), (2048, 3001), (64, 10))]
I8_GRID += [(1 << 20, 1000, 64, 1024), (17, 300, 70, 10), (1, 1, 1, 1), (4096, 1_000_000, 256, 10)]
I8_CAPS = (None, "64", "100")


def shard_plan_cases():
    for devs in DEVICE_LISTS:
        for m, n, d, k in SHAPES:
            for compute in (0, 1):
                for host_rows in (True, False):
                    for metric in (0, 1, 2):
                        yield devs, m, n, d, k, metric, compute, host_rows


def shard_plan_key(devs, m, n, d, k, metric, compute, host_rows):
    return f"{','.join(map(str, devs))}|{m}x{n}x{d} k={k} metric={metric} compute={compute} host={int(host_rows)}"


def shard_plan_now(case):
    from polars_matmul import _native

    devs, m, n, d, k, metric, compute, host_rows = case
    plan_of, plans, offs = _native.shard_plan(devs, m, n, d, k, metric, compute, host_rows)
    return {"plan_of": plan_of, "plan_dev": [p[0] for p in plans], "plan_bytes": [p[1] for p in plans],
            "list_offsets": offs}


def i8_key(m, n, d, k, cap):
    return f"{m}x{n}x{d} k={k} cap={cap}"


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(os.environ):
        if name.startswith("PMM_"):
            monkeypatch.delenv(name)
    return monkeypatch


def test_shard_plan_unchanged(clean_env):
    want = json.load(open(SHARD_PLAN))
    cases = list(shard_plan_cases())
    assert len(want) == len(cases) == len(DEVICE_LISTS) * len(SHAPES) * 12
    for case in cases:
        assert shard_plan_now(case) == want[shard_plan_key(*case)], shard_plan_key(*case)


def test_shard_plan_golden_covers_short_shards_and_widened_bf16():
    want = json.load(open(SHARD_PLAN))
    short = want[shard_plan_key([0] * 8, 37, 100, 40, 64, 0, 0, True)]
    assert short["plan_of"] == [0] * 8 and len(set(short["list_offsets"])) == 8  # 12 or 13 rows each, k = 64
    wide = want[shard_plan_key([0], 256, 16384, 1024, 100, 0, 1, False)]
    # the widened route keeps f32 images of Q and C (d = 1024 floats a row) in the shard's workspace
    assert wide["plan_bytes"][0] > (256 + 16384) * 1024 * 4


def test_i8_workspace_bytes_unchanged(clean_env):
    from polars_matmul import _native

    want = json.load(open(WORKSPACE_I8))
    assert len(want) == len(I8_GRID) * len(I8_CAPS) * 3
    for cap in I8_CAPS:
        if cap is None:
            clean_env.delenv("PMM_I8_CAP", raising=False)
        else:
            clean_env.setenv("PMM_I8_CAP", cap)
        for m, n, d, k in I8_GRID:
            for metric in (0, 1, 2):
                assert _native.i8_workspace_bytes(m, n, d, k, metric) == want[i8_key(m, n, d, k, cap) + f" metric={metric}"]


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "polars-matmul_amd"))
    from polars_matmul import _native

    for name in list(os.environ):
        if name.startswith("PMM_") and name != "PMM_LIB":
            del os.environ[name]
    json.dump({shard_plan_key(*c): shard_plan_now(c) for c in shard_plan_cases()}, open(SHARD_PLAN, "w"), indent=0,
              sort_keys=True)
    out = {}
    for cap in I8_CAPS:
        os.environ.pop("PMM_I8_CAP", None)
        if cap is not None:
            os.environ["PMM_I8_CAP"] = cap
        for m, n, d, k in I8_GRID:
            for metric in (0, 1, 2):
                out[i8_key(m, n, d, k, cap) + f" metric={metric}"] = _native.i8_workspace_bytes(m, n, d, k, metric)
    json.dump(out, open(WORKSPACE_I8, "w"), indent=0, sort_keys=True)
    print(f"recorded {len(list(shard_plan_cases()))} shard plans and {len(out)} int8 workspace sizes")
