"""Wall time of short host calls (median of REPS after warm-up), one JSON line."""
import json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "polars-matmul_amd"))
from polars_matmul import _native
REPS = 300
def med(fn):
    for _ in range(20):
        fn()
    xs = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); xs.append((time.perf_counter() - t) * 1e6)
    return round(statistics.median(xs), 2)
rs = np.random.RandomState(1)
q = rs.randn(1000, 256).astype(np.float32); c = rs.randn(10000, 256).astype(np.float32)
out = {"lib": os.environ.get("PMM_LIB", "libpmm.so")}
out["f32_host_c1_us"] = med(lambda: _native.topk_host(q, c, 10, 0))
h = _native.DeviceCorpus(c); out["f32_handle_c1_us"] = med(lambda: h.topk(q, 10, 0)); h.close()
q64, c64 = q[:256].astype(np.float64), c.astype(np.float64)
h = _native.DeviceCorpus(c64); out["f64_handle_256x10000x256_us"] = med(lambda: h.topk(q64, 10, 0)); h.close()
q8 = rs.randint(-128, 128, size=(256, 256)).astype(np.int8); c8 = rs.randint(-128, 128, size=(10000, 256)).astype(np.int8)
h = _native.DeviceCorpus.int8(c8); out["i8_handle_256x10000x256_us"] = med(lambda: h.topk(q8, 10, 0)); h.close()
hb = _native.DeviceCorpus(c, compute="bf16"); out["bf16_handle_c1_us"] = med(lambda: hb.topk(q, 10, 0)); hb.close()
import torch
pr = torch.cuda.get_device_properties(0)
out["device"] = pr.name; out["max_clock_mhz"] = getattr(pr, "clock_rate", 0) / 1000
print(json.dumps(out))
