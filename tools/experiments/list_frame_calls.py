"""Wall time of short list-valued host calls (range, self range, candidates,
grouped; median of REPS after warm-up), one JSON line.  PMM_PKG names the
directory holding the polars_matmul package to load (default: this tree's), so a
parent checkout's package and library can be measured by the same script."""
import json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("PMM_PKG", os.path.join(ROOT, "polars-matmul_amd")))
from polars_matmul import _native
REPS = 300
COS = _native.METRIC_COSINE
def med(fn):
    for _ in range(20):
        fn()
    xs = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); xs.append((time.perf_counter() - t) * 1e6)
    return round(statistics.median(xs), 2)
def unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)
rs = np.random.RandomState(1)
q = rs.randn(256, 256).astype(np.float32); c = rs.randn(10000, 256).astype(np.float32)
out = {"pkg": os.environ.get("PMM_PKG", "tree"), "lib": os.path.basename(_native.LIB_PATH)}
h = _native.DeviceCorpus(c)
t = float(np.sort((unit(q) @ unit(c).T).reshape(-1))[-2560])  # about 10 hits per row
out["range_256x10000x256_us"] = med(lambda: h.range(q, t, COS))
offsets = np.arange(257, dtype=np.int64) * 100
ids = np.concatenate([np.sort(rs.choice(10000, 100, replace=False)) for _ in range(256)]).astype(np.uint32)
out["candidates_256x100_k10_us"] = med(lambda: h.topk_candidates(q, offsets, ids, 10, COS))
hp = h.partition(rs.randint(0, 100, size=10000).astype(np.uint32), 100)
ql = rs.randint(0, 100, size=256).astype(np.uint32)
out["grouped_256q_100labels_k10_us"] = med(lambda: hp.topk_grouped(q, ql, 10, COS))
hp.close(); h.close()
cs = c[:4096]
h = _native.DeviceCorpus(cs)
s = unit(cs) @ unit(cs).T
ts = float(np.sort(s[np.triu_indices(4096, 1)])[-40960])  # about 10 pairs per row
out["self_range_4096x256_us"] = med(lambda: h.range_self(ts, COS))
h.close()
print(json.dumps(out))
