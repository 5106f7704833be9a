"""The device-resident entries as a table of cases, with one way to run each.

tests/test_gpu_stream_order.py and tests/test_gpu_min_alignment.py vary what a caller of the
thirteen entries that take a `void *stream` controls and the value tests never vary: the stream,
and the layout of the operands, outputs and workspace ("Streams and alignment").
Both run the same cases through the same code, which lives here:

  Operand   host rows and the byte image of those rows at a row stride, with a poison byte in
            every position the entry may not read (0xFF: an all-ones f32, f64 or bf16 is a NaN;
            0x7F for integer rows) and zeros where the entry wants zero padding
  Output    name, dtype, shape and the weakest base alignment the entry takes
  Case      operands, outputs, workspace size, the call and a truth computed on the CPU
  Placed    device bytes between guard bands, starting `off` bytes past a 256-byte boundary
  run_case  one synchronous call at the tight or the weak layout, bands checked
  baseline  the tight call on the null stream, once per case: the reference of the outputs
            that have no CPU truth (bf16 lists, reciprocals, rel / unsafe)

The shapes are those of tests/test_gpu_dirty_scratch.py, the smallest that take each route.
Nothing here touches a GPU at import.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle
import polars_matmul
from polars_matmul import _native
from test_bits_cpu import hamming_truth
from test_gpu_dirty_scratch import EMPTY_IDX, EMPTY_SCORE, SCREEN_ON, Banded, assert_same, roundup

COS, DOT, EUC = _native.METRIC_COSINE, _native.METRIC_DOT, _native.METRIC_EUCLIDEAN
F32, BF16 = _native.COMPUTE_F32, _native.COMPUTE_BF16
NAN_BYTE, INT_BYTE = 0xFF, 0x7F   # poison of float and of integer rows
OUT_FILL = 0x5A                   # what an output holds before the call
WS_FILL = 0xFF                    # what a caller's workspace holds before the call


def bf16_bits(a):
    """f32 rows rounded to bf16 by torch's cast (round to nearest even): the bit patterns, uint16."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


class Operand:
    """`data` (rows x d elements) as an entry reads it: at row stride tight_ld or weak_ld, columns
    d .. roundup(d, pad) - 1 zero, at a 256-byte boundary (tight) or weak_off bytes past one."""

    def __init__(self, name, data, pad, poison, weak_ld, weak_off=16, fixed_ld=None):
        self.name, self.data = name, np.ascontiguousarray(data)
        (self.rows, self.d), self.elem = self.data.shape, self.data.dtype.itemsize
        self.pad, self.poison = pad, poison
        self.tight_ld = fixed_ld or roundup(self.d, pad)
        self.weak_ld, self.weak_off = fixed_ld or weak_ld, weak_off

    def nbytes(self, ld):
        return self.rows * ld * self.elem

    def image(self, ld):
        img = np.full((self.rows, ld * self.elem), self.poison, np.uint8)
        img[:, :roundup(self.d, self.pad) * self.elem] = 0
        img[:, :self.d * self.elem] = self.data.view(np.uint8).reshape(self.rows, self.d * self.elem)
        return img.reshape(-1)

    def poisoned(self):
        """The operand with the poison in place of its rows: what a call reads that does not wait
        for its producer."""
        rows = np.full((self.rows, self.d * self.elem), self.poison, np.uint8).view(self.data.dtype)
        return Operand(self.name, rows, self.pad, self.poison, self.weak_ld, self.weak_off)


class Output:
    def __init__(self, name, dtype, shape, weak_off, zeroed=False):
        self.name, self.dtype, self.shape, self.weak_off = name, np.dtype(dtype), tuple(shape), weak_off
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.zeroed = zeroed  # the caller zeroes it before the call, on the call's stream


class Case:
    """blocks: the entry synchronises the stream by design on this route (pmm.h lists the
    places).  arena: the entry takes no workspace argument and uses the thread's arena."""

    def __init__(self, name, kind, make, outputs, call, truth, knobs=None, workspace=None, blocks=False, arena=False,
                 compute=None):
        self.name, self.kind, self.knobs = name, kind, dict(knobs or {})
        self._make, self.outputs, self._call, self._truth = make, outputs, call, truth
        self._workspace, self.blocks, self.arena, self.compute = workspace, blocks, arena, compute

    def __repr__(self):
        return self.name

    @functools.cached_property
    def operands(self):
        return self._make()

    def operand(self, name):
        return next(op for op in self.operands if op.name == name)

    def workspace_bytes(self):
        """With the case's knobs in the environment.  0: the entry takes no workspace."""
        return self._workspace() if self._workspace else 0

    def call(self, p, o, ws, stream):
        """p: operand name -> (pointer, row stride); o: output name -> pointer; ws: (pointer, bytes),
        (0, 0) for the thread's arena; stream: a HIP stream handle, 0 for the null stream."""
        self._call(p, o, ws, stream)

    @functools.cached_property
    def truth(self):
        """Output name -> array, from the CPU alone; the outputs it leaves out come from baseline()."""
        return self.truth_of(self.operands)

    def truth_of(self, operands):
        return self._truth({op.name: op.data for op in operands})


# ---------------------------------------------------------------------------
# The top-k entries
# ---------------------------------------------------------------------------
# kind -> (pad, poison, weak stride above the padded width, score dtype, weak offset of the scores)
TOPK_KINDS = {"f32": (32, NAN_BYTE, 4, np.float32, 4), "bf16": (128, NAN_BYTE, 8, np.float32, 4),
              "f64": (16, NAN_BYTE, 2, np.float64, 8), "i8": (64, INT_BYTE, 16, np.float64, 8),
              "bits": (16, INT_BYTE, 16, np.float64, 8)}


def topk_case(name, kind, m, n, d, k, metric=COS, knobs=None, blocks=False):
    pad, poison, extra, sdt, soff = TOPK_KINDS[kind]

    def make():
        rs = np.random.RandomState(m + n + d + k)
        if kind == "i8":
            q, c = (rs.randint(-128, 128, size=(r, d)).astype(np.int8) for r in (m, n))
        elif kind == "bits":
            q, c = (rs.randint(0, 256, size=(r, d)).astype(np.uint8) for r in (m, n))
        else:
            dt = np.float64 if kind == "f64" else np.float32
            q, c = rs.randn(m, d).astype(dt), rs.randn(n, d).astype(dt)
            if kind == "bf16":
                q, c = bf16_bits(q), bf16_bits(c)
        return [Operand(nm, a, pad, poison, roundup(d, pad) + extra) for nm, a in (("q", q), ("c", c))]

    def truth(rows):
        q, c = rows["q"], rows["c"]
        if kind == "bf16":
            return {}  # (no CPU statement of the bf16 path: the lists are deterministic, see baseline)
        if kind == "bits":
            idx, sc = hamming_truth(q, c, k)
        else:
            wide = np.float64 if kind == "i8" else q.dtype
            idx, sc = oracle.topk(q.astype(wide), c.astype(wide), k, metric)
        return {"idx": np.asarray(idx).astype(np.uint32), "score": np.asarray(sc).astype(sdt)}

    def nat():
        """The binding the case calls: the product's, or a second library's (case.native)."""
        return case.native or _native

    def call(p, o, ws, stream):
        (pq, ldq), (pc, ldc) = p["q"], p["c"]
        if kind == "f64":
            _native.topk_f64_device(pq, ldq, m, pc, ldc, n, d, k, metric, o["idx"], o["score"], stream=stream)
        elif kind == "bits":
            _native.topk_bits_device(pq, ldq, m, pc, ldc, n, d, k, o["idx"], o["score"], workspace=ws[0],
                                     workspace_bytes=ws[1], stream=stream)
        else:
            fn = {"f32": nat().topk_device, "bf16": nat().topk_bf16_device, "i8": nat().topk_i8_device}[kind]
            fn(pq, ldq, m, pc, ldc, n, d, k, metric, o["idx"], o["score"], workspace=ws[0], workspace_bytes=ws[1],
               stream=stream)

    workspace = {"f32": lambda: nat().workspace_bytes(m, n, d, k, metric, F32),
                 "bf16": lambda: nat().workspace_bytes(m, n, d, k, metric, BF16),
                 "i8": lambda: _native.i8_workspace_bytes(m, n, d, k, metric),
                 "bits": lambda: _native.bits_workspace_bytes(m, n, d, k), "f64": None}[kind]
    case = Case(name, kind, make, [Output("idx", np.uint32, (m, k), 4), Output("score", sdt, (m, k), soff)], call, truth,
                knobs, workspace, blocks or kind in ("i8", "bits"), arena=kind == "f64",
                compute={"f32": F32, "bf16": BF16}.get(kind))
    case.shape, case.native = (m, n, d, k, metric), None
    return case


F32_FUSED = topk_case("f32 fused cosine", "f32", 130, 5003, 37, 10, COS)
F32_SCREENED = topk_case("f32 screened", "f32", 70, 3037, 256, 10, COS, SCREEN_ON, blocks=True)
F64_MATERIALISED = topk_case("f64 materialised", "f64", 33, 1037, 37, 10, EUC, {"PMM_F64_FUSED": "0"})
INT8 = topk_case("int8", "i8", 33, 3001, 70, 10, COS)
BITS = topk_case("bits", "bits", 33, 1037, 9, 10)
BF16_WS = topk_case("bf16 wave-specialised k=100", "bf16", 130, 16384, 256, 100, COS)
BF16_WIDENED = topk_case("bf16 widened d=1024", "bf16", 70, 3000, 1024, 100, COS)
F64_FUSED = topk_case("f64 fused", "f64", 33, 1037, 37, 10, COS, {"PMM_F64_FUSED": "1"}, blocks=True)
TOPK_CASES = [
    F32_FUSED,
    topk_case("f32 fused dot", "f32", 130, 5000, 256, 10, DOT),
    topk_case("f32 materialised k=1025", "f32", 64, 4099, 256, 1025, DOT),
    topk_case("f32 global sort k=3000", "f32", 33, 8192, 96, 3000, COS),
    # the materialised row-chunk loop past its first chunk: three chunks of 24, 24 and 16 rows
    # (PMM_MATERIALISE_BUDGET = 24 rows of 4099 f32 scores, tests/row_chunk_cases.py)
    topk_case("f32 materialised k=1025 in row chunks", "f32", 64, 4099, 256, 1025, DOT,
              {"PMM_MATERIALISE_BUDGET": str(24 * 4099 * 4)}),
    F32_SCREENED,
    BF16_WS,
    topk_case("bf16 one-wave k=500", "bf16", 70, 5000, 96, 500, EUC),
    BF16_WIDENED,
    F64_FUSED,
    F64_MATERIALISED,
    INT8,
    BITS,
]
# an odd k: output rows that are only 4-byte aligned
F32_K7 = topk_case("f32 fused k=7", "f32", 130, 5003, 37, 7, COS)
ODD_K_CASES = [F32_K7, topk_case("bf16 one-wave k=7", "bf16", 70, 5000, 96, 7, EUC)]
# the three fills of the fused f32 path and the unseeded bf16 one (test_gpu_dirty_scratch.WORKSPACE_CASES)
FILL_CASES = [
    topk_case("f32 cosine unseeded", "f32", 130, 5000, 96, 10, COS, {"PMM_SEED": "0"}),
    topk_case("f32 cosine seeded", "f32", 130, 5000, 96, 10, COS, {"PMM_SEED": "1"}),
    topk_case("f32 cosine seeded by the GEMM", "f32", 130, 5000, 96, 10, COS, {"PMM_SEED": "1", "PMM_SEED_GEMM": "1"}),
    topk_case("f32 dot unseeded", "f32", 130, 5000, 256, 10, DOT, {"PMM_SEED": "0"}),
    topk_case("f32 dot seeded", "f32", 130, 5000, 256, 10, DOT, {"PMM_SEED": "1"}),
    topk_case("f32 dot seeded by the GEMM", "f32", 130, 5000, 256, 10, DOT, {"PMM_SEED": "1", "PMM_SEED_GEMM": "1"}),
    topk_case("bf16 unseeded", "bf16", 130, 16384, 256, 100, COS, {"PMM_BF16_SEED": "0"}),
]


# ---------------------------------------------------------------------------
# The row entries: sign packing, norms, rounding, the screen's preparation
# ---------------------------------------------------------------------------
def pack_case():
    rows, d = 70, 65
    w = -(-d // 8)
    ld_out = roundup(w, 8)

    def make():
        x = np.random.RandomState(65).randn(rows, d).astype(np.float32)
        x[::7, ::5] = 0.0
        x[1::7, ::5] = -0.0
        # any 4-byte-aligned address, any stride >= d
        return [Operand("x", x, 1, NAN_BYTE, d + 1, weak_off=4)]

    def truth(r):
        want = np.zeros((rows, ld_out), np.uint8)  # (each row's roundup(ceil(d / 8), 8) bytes are written whole)
        want[:, :w] = polars_matmul.pack_sign(r["x"])
        return {"packed": want}

    def call(p, o, ws, stream):
        _native.pack_sign_device(p["x"][0], p["x"][1], rows, d, o["packed"], ld_out, stream=stream)

    # 8-byte aligned and not 16
    return Case("pack_sign", "pack", make, [Output("packed", np.uint8, (rows, ld_out), 8)], call, truth)


def norms_case(f64):
    rows, d = 70, 37
    dt = np.float64 if f64 else np.float32
    squared = f64  # (the f32 case takes the root, the f64 case the sum)

    def make():
        a = np.random.RandomState(37 + f64).randn(rows, d).astype(dt)
        # an odd stride at the element's own alignment
        return [Operand("a", a, 1, NAN_BYTE, d + 2, weak_off=dt().itemsize)]

    def call(p, o, ws, stream):
        _native.norms_device(p["a"][0], p["a"][1], rows, d, squared, o["norms"], f64=f64, stream=stream)

    return Case("norms f64" if f64 else "norms f32", "norms", make, [Output("norms", dt, (rows,), dt().itemsize)], call,
                lambda r: {"norms": oracle.norms(r["a"], squared)})


def rounding_case(entry):
    rows, d = 70, 200
    ldo = roundup(d, 128)
    arrays = ("norm", "inv_norm", "sq", "sq_factor") if entry == "round" else ("norm", "inv_norm", "rel", "unsafe")

    def make():
        a = np.random.RandomState(200).randn(rows, d).astype(np.float32)
        return [Operand("a", a, 1, NAN_BYTE, d + 1, weak_off=4)]  # (any alignment: an odd stride at + 4 bytes)

    def truth(r):
        a = r["a"]
        bits_ = np.zeros((rows, ldo), np.uint16)
        bits_[:, :d] = bf16_bits(a)
        out = {"rows": bits_}
        if entry == "round":
            # the norms of the ROUNDED rows widened to f32
            wide = np.ascontiguousarray((bits_[:, :d].astype(np.uint32) << 16).view(np.float32))
            out["norm"], out["sq"] = oracle.norms(wide, False), oracle.norms(wide, True)
        else:
            out["norm"] = oracle.norms(a, False)  # (of the unrounded row)
        return out

    def call(p, o, ws, stream):
        pa, ld = p["a"]
        if entry == "round":
            _native.round_bf16_device(pa, ld, rows, d, o["rows"], ldo, norm=o["norm"], inv_norm=o["inv_norm"], sq=o["sq"],
                                      sq_factor=o["sq_factor"], stream=stream)
        else:
            _native.screen_prepare_device(pa, ld, rows, d, o["rows"], ldo, norm=o["norm"], inv_norm=o["inv_norm"],
                                          rel=o["rel"], unsafe=o["unsafe"], scalars=o["scalars"], stream=stream)

    outs = [Output("rows", np.uint16, (rows, ldo), 16)] + [Output(nm, np.uint32, (rows,), 4) for nm in arrays]
    if entry == "prepare":
        outs.append(Output("scalars", np.uint32, (2,), 4, zeroed=True))

    def as_bits(t):
        return {nm: np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype) for nm, a in t.items()}

    return Case(entry, "rounding", make, outs, call, lambda r: as_bits(truth(r)))


# ---------------------------------------------------------------------------
# The three merge entries (test_gpu_dirty_scratch.test_merge_entries_inside_guard_bands)
# ---------------------------------------------------------------------------
def merge_case(entry):
    m, lists, k_in, k_out = 37, 5, 40, 100
    strided = entry != "merge"
    row_stride, list_stride = (lists * (k_in + 8) + 16, k_in + 8) if strided else (lists * k_in, k_in)

    def lists_of():
        rs = np.random.RandomState(5)
        idx = np.stack([np.concatenate([g * 4096 + rs.permutation(4096)[:k_in] for g in range(lists)]) for _ in range(m)])
        idx = idx.reshape(m, lists, k_in).astype(np.uint32)
        sc = rs.randn(m, lists, k_in).astype(np.float32)
        order = np.argsort(-sc, axis=2, kind="stable")  # every list best first
        idx, sc = np.take_along_axis(idx, order, 2), np.take_along_axis(sc, order, 2)
        idx[:, 1, k_in - 5:] = EMPTY_IDX  # a list with empty slots at its end
        sc[:, 1, k_in - 5:] = np.nan
        return idx, sc

    def make():
        idx, sc = lists_of()
        if not strided:
            ti, ts = idx.reshape(m, -1), sc.reshape(m, -1)
        else:
            # slack between rows and lists that holds winning entries (index 7, score +inf for cosine)
            ti = np.full((m + 1, row_stride), 7, np.uint32)
            ts = np.full((m + 1, row_stride), np.inf, np.float32)
            for g in range(lists):
                ti[:m, g * list_stride:g * list_stride + k_in] = idx[:, g]
                ts[:m, g * list_stride:g * list_stride + k_in] = sc[:, g]
        return [Operand("idx", ti, 1, INT_BYTE, None, weak_off=4, fixed_ld=row_stride),
                Operand("score", ts, 1, NAN_BYTE, None, weak_off=4, fixed_ld=row_stride)]

    def truth(r):
        # the k_out best of a row's entries, score descending, then index ascending
        take = np.concatenate([np.arange(k_in) + g * list_stride for g in range(lists)])
        fi, fs = r["idx"][:m, take], r["score"][:m, take]
        want_i = np.full((m, k_out), EMPTY_IDX, np.uint32)
        want_s = np.full((m, k_out), EMPTY_SCORE, np.uint32).view(np.float32)
        for row in range(m):
            ok = fi[row] != EMPTY_IDX
            o = np.lexsort((fi[row][ok], -fs[row][ok]))[:k_out]
            want_i[row, :o.size], want_s[row, :o.size] = fi[row][ok][o], fs[row][ok][o]
        return {"idx": want_i, "score": want_s}

    def call(p, o, ws, stream):
        if not strided:
            _native.merge_device(p["idx"][0], p["score"][0], m, lists, k_in, k_out, COS, o["idx"], o["score"], stream)
        else:
            _native.merge_strided_device(p["idx"][0], p["score"][0], m, lists, k_in, row_stride, list_stride, k_out, COS,
                                         o["idx"], o["score"], stream, sorted_lists=entry == "sorted strided merge")

    return Case(entry, "merge", make, [Output("idx", np.uint32, (m, k_out), 4), Output("score", np.float32, (m, k_out), 4)],
                call, truth)


ROW_CASES = [pack_case(), norms_case(False), norms_case(True), rounding_case("round"), rounding_case("prepare"),
             merge_case("merge"), merge_case("strided merge"), merge_case("sorted strided merge")]
CASES = TOPK_CASES + ROW_CASES


# ---------------------------------------------------------------------------
# Device memory and the call
# ---------------------------------------------------------------------------
class Placed:
    """`nbytes` of device memory starting `off` bytes past a 256-byte boundary, between guard bands
    (test_gpu_dirty_scratch.Banded); the `off` bytes before it hold `fill` and are checked too."""

    def __init__(self, nbytes, off=0, fill=OUT_FILL):
        self.b, self.off, self.nbytes, self.fill = Banded(nbytes + off, fill=fill), off, nbytes, fill
        self.ptr = self.b.ptr + off
        assert self.b.ptr % 256 == 0 and self.ptr % 256 == off % 256

    @property
    def view(self):
        """The bytes as a uint8 tensor (a view: copies into it land in place)."""
        return self.b.t[self.b.lo + self.off:self.b.hi]

    def array(self, dtype, shape):
        return self.view.cpu().numpy().view(dtype).reshape(shape)

    def check(self, label):
        import torch

        self.b.check(label)
        assert bool(torch.all(self.b.t[self.b.lo:self.b.lo + self.off] == self.fill)), \
            f"{label}: the {self.off} bytes between the boundary and the buffer were written"


def apply_knobs(env, case):
    for name, value in case.knobs.items():
        env.setenv(name, value)
    if case.knobs.get("PMM_F32_SCREEN") == "1":
        # (the screened route's workspace holds the images and the re-run's bytes)
        m, n, d, k, metric = case.shape
        here = _native.workspace_bytes(m, n, d, k, metric, F32)
        env.setenv("PMM_F32_SCREEN", "0")
        assert here > _native.workspace_bytes(m, n, d, k, metric, F32), f"{case.name}: the call does not screen"
        env.setenv("PMM_F32_SCREEN", "1")


def place_wide(op, ld, whole=False):
    """The operand at a row stride whose image no host holds: one device allocation filled on the
    device with the poison, then the rows with their zero padding written through a strided view
    from the tight host rows.  The last row ends at its padded width (a column slice of a wide
    matrix), so the guard band starts right behind it; whole: the last row has its stride too."""
    import torch

    width = roundup(op.d, op.pad) * op.elem
    assert ld * op.elem >= width
    pl = Placed((op.rows - 1) * ld * op.elem + (ld * op.elem if whole else width), 0, fill=op.poison)
    tight = np.zeros((op.rows, width), np.uint8)
    tight[:, :op.d * op.elem] = op.data.view(np.uint8).reshape(op.rows, op.d * op.elem)
    torch.as_strided(pl.view, (op.rows, width), (ld * op.elem, 1)).copy_(torch.from_numpy(tight))
    return pl


def place_operands(case, weak, filled=True, wide=None):
    """Operand name -> (Placed, row stride).  filled: the rows are there (a synchronous upload);
    else every byte is the poison and the caller produces the rows.  wide: operand name -> row
    stride, placed by place_wide."""
    import torch

    out = {}
    for op in case.operands:
        if wide and op.name in wide:
            out[op.name] = (place_wide(op, wide[op.name], getattr(case, "whole_rows", False)), wide[op.name])
            continue
        ld = op.weak_ld if weak else op.tight_ld
        pl = Placed(op.nbytes(ld), op.weak_off if weak else 0, fill=op.poison)
        if filled:
            pl.view.copy_(torch.from_numpy(op.image(ld)))
        out[op.name] = (pl, ld)
    return out


def place_outputs(case, weak):
    return {o.name: Placed(o.nbytes, o.weak_off if weak else 0, fill=OUT_FILL) for o in case.outputs}


def place_workspace(case, off=0):
    """A caller's workspace of exactly workspace_bytes() filled with 0xFF; None when the entry takes none."""
    wb = case.workspace_bytes()
    return Placed(wb, off, fill=WS_FILL) if wb else None


def ws_args(ws):
    return (ws.ptr, ws.nbytes) if ws is not None else (0, 0)


def call_placed(case, ops, outs, ws, stream):
    case.call({nm: (pl.ptr, ld) for nm, (pl, ld) in ops.items()}, {nm: pl.ptr for nm, pl in outs.items()}, ws_args(ws),
              stream)


def read_outputs(case, outs):
    return {o.name: outs[o.name].array(o.dtype, o.shape) for o in case.outputs}


def check_bands(case, ops, outs, ws, label):
    for nm, (pl, _) in ops.items():
        pl.check(f"{label} operand {nm}")
    for nm, pl in outs.items():
        pl.check(f"{label} output {nm}")
    if ws is not None:
        ws.check(f"{label} workspace")


def run_case(case, weak=False, weak_operands=None, ws_off=None, arena=False, stream=0, wide=None):
    """One synchronous call.  weak: operands and outputs at the weakest layout (weak_operands
    overrides it for the operands alone); ws_off: the workspace's offset from a 256-byte boundary
    (default 16 when weak, for the entries that take it there); arena: workspace = NULL; wide:
    operand name -> row stride of the operands placed on the device (place_wide)."""
    import torch

    weak_ops = weak if weak_operands is None else weak_operands
    ops, outs = place_operands(case, weak_ops, wide=wide), place_outputs(case, weak)
    if ws_off is None:
        ws_off = 16 if weak and case.kind in ("f32", "bf16") else 0
    ws = None if arena else place_workspace(case, ws_off)
    for o in case.outputs:
        if o.zeroed:
            outs[o.name].view.zero_()
    torch.cuda.synchronize()
    call_placed(case, ops, outs, ws, stream)
    torch.cuda.synchronize()
    check_bands(case, ops, outs, ws, case.name)
    return read_outputs(case, outs)


_BASELINE = {}


def baseline(case):
    """The case on the null stream with tight, 256-byte-aligned operands, once per process (the
    case's knobs must be in the environment)."""
    if case.name not in _BASELINE:
        _BASELINE[case.name] = run_case(case)
    return _BASELINE[case.name]


def expected(case):
    """Every output's expected array: the CPU truth where there is one, else the baseline's."""
    want = dict(baseline(case))
    want.update(case.truth)
    return want


def assert_outputs(case, got, want, label):
    names = [o.name for o in case.outputs]
    assert_same(tuple(got[nm] for nm in names), tuple(want[nm] for nm in names), f"{case.name}: {label}")


def assert_untouched(outs, label):
    import torch

    for nm, pl in outs.items():
        assert bool(torch.all(pl.view == pl.fill)), f"{label}: output {nm} was written"
        pl.check(f"{label} output {nm}")
