"""CPU side of the bf16 corpus handle and ``compute=`` on ``.pmm.topk``: the
handle's footprint formula, the compute-mode check of ``_topk`` (before any
device work), the namespace forwarding the keyword (against the stand-in
``polars`` of tests/test_namespace.py's kind, in a subprocess), and the
one-pass round-and-norm kernel's resources (hipcc cross-compiles gfx950 here)."""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from isa_util import CSRC, FLAGS, HIPCC, have_hipcc
from polars_matmul import _native
from polars_matmul._polars_matmul import _topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d, dp", [(1, 128), (128, 128), (129, 256), (768, 768)])
def test_bf16_corpus_device_bytes(d, dp):
    n = 1000
    # bf16 rows at stride roundup(d, 128) + four f32 arrays per row, whatever the host dtype
    want = n * dp * 2 + 16 * n
    assert _native.corpus_device_bytes(n, d, np.float32, compute="bf16") == want
    assert _native.corpus_device_bytes(n, d, np.float64, compute="bf16") == want
    assert _native.corpus_device_bytes(n, d, np.float32, "f32") == _native.corpus_device_bytes(n, d, np.float32)
    assert _native.DTYPE_BF16 == 2


def test_bf16_handle_is_smaller_than_f32_at_10m_x_1024():
    f32 = _native.corpus_device_bytes(10_000_000, 1024, np.float32)
    bf16 = _native.corpus_device_bytes(10_000_000, 1024, np.float32, compute="bf16")
    assert f32 == 10_000_000 * (1024 * 4 + 16) and bf16 == 10_000_000 * (1024 * 2 + 16)


def test_unknown_compute_raises_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the compute check")

    for name in ("topk_host", "DeviceCorpus", "device_memory", "get_devices", "metric_from_str"):
        monkeypatch.setattr(_native, name, boom)
    q = np.zeros((2, 4), dtype=np.float32)
    with pytest.raises(ValueError) as ei:
        _topk(q, q, 1, "cosine", compute="fp8")
    # the numpy-level topk's text
    assert str(ei.value) == "compute must be 'f32' or 'bf16', not 'fp8'"
    import polars_matmul

    with pytest.raises(ValueError) as ej:
        polars_matmul.topk(q, q, 1, compute="fp8")
    assert str(ej.value) == str(ei.value)
    with pytest.raises(ValueError):
        _native.corpus_device_bytes(1, 1, np.float32, compute="fp8")


NAMESPACE_SCRIPT = r'''
import json, sys, types
sys.path.insert(0, %(pkg)r)
pl = types.ModuleType("polars")
pl.UInt32, pl.Float32, pl.Float64 = "u32", "f32", "f64"
pl.List = lambda inner: ("List", inner)
pl.Struct = lambda fields: ("Struct", tuple(fields.items()))
pl.Array = lambda inner, n: ("Array", inner, n)
class Expr:
    def __init__(self):
        self.calls = []
    def map_batches(self, fn, **kw):
        self.calls.append((fn, kw))
        return ("mapped", kw)
class Series:
    def __init__(self, values):
        self.values = values
    def __len__(self):
        return len(self.values)
registry = {}
def register_expr_namespace(name):
    def deco(cls):
        registry[name] = cls
        return cls
    return deco
pl.Expr, pl.Series = Expr, Series
pl.api = types.SimpleNamespace(register_expr_namespace=register_expr_namespace)
sys.modules["polars"] = pl

import polars_matmul
calls = []
def rec(s, c, k, m, *args, **kw):
    calls.append([s, len(c), k, m, list(args), kw])
    return "topk-result"
polars_matmul._topk = rec
ns = registry["pmm"]
corpus = Series([[1.0, 0.0]] * 3)
out = {}
e = Expr(); ns(e).topk(corpus, 2, "dot", compute="bf16"); out["r"] = e.calls[0][0]("b0"); out["bf16"] = calls[-1]
e = Expr(); ns(e).topk(corpus, 5, "euclidean", "bf16"); e.calls[0][0]("b1"); out["bf16_pos"] = calls[-1]
e = Expr(); ns(e).topk(corpus, 2, "dot"); e.calls[0][0]("b2"); out["default"] = calls[-1]
e = Expr(); ns(e).topk(corpus, k=4, compute="f32"); e.calls[0][0]("b3"); out["f32"] = calls[-1]
try:
    ns(Expr()).topk(corpus, 2, compute="fp8")
    out["bad"] = None
except ValueError as err:
    out["bad"] = str(err)
print(json.dumps(out))
'''


def test_namespace_forwards_compute_to_topk():
    code = NAMESPACE_SCRIPT % {"pkg": os.path.join(ROOT, "polars-matmul_amd")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["r"] == "topk-result"
    assert out["bf16"] == ["b0", 3, 2, "dot", [], {"compute": "bf16"}]
    assert out["bf16_pos"] == ["b1", 3, 5, "euclidean", [], {"compute": "bf16"}]
    # the first three arguments stay positional and the default call is the reference's four-argument one
    assert out["default"] == ["b2", 3, 2, "dot", [], {}]
    assert out["f32"] == ["b3", 3, 4, "cosine", [], {}]
    assert out["bad"] == "compute must be 'f32' or 'bf16', not 'fp8'"


@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_round_norms_kernel_uses_no_scratch_and_modest_lds():
    # the kernel carries 8 rounded values, the row's partial sum and up to 7
    # tail values per lane: all of it must stay in registers (a scratch access
    # per group would sit in the one pass over the rows), with the LDS band
    # small enough for 8 workgroups per CU
    from test_kernel_resources import scratch_by_kernel

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bf16.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_bf16.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = {k: v for k, v in scratch_by_kernel(asm).items() if "round_norms_bf16_kernel" in k}
    assert len(sc) == 1, sorted(sc)
    assert list(sc.values()) == [(0, 0)], f"scratch (bytes, instructions): {sc}"
    name = next(iter(sc))
    body = asm.split(f".amdhsa_kernel {name}")[1].split(".end_amdhsa_kernel")[0]
    lds = [int(l.split()[1]) for l in body.splitlines() if l.strip().startswith(".amdhsa_group_segment_fixed_size")]
    assert lds and 0 < lds[0] <= 20 * 1024, lds
    # the rows leave as 16-byte stores
    func = asm.split(f"\n{name}:")[1].split("s_endpgm")[0]
    assert "global_store_dwordx4" in func
