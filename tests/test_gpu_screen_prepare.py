"""GPU tests of ``pmm_screen_prepare_device`` alone, on torch tensors: the one
pass that prepares f32 rows for the screened cosine top-k (bf16 image, exact
norm and factor of the unrounded row, residual bound, unsafe flag, and the
scalar pair a corpus image build reads back).

References are independent of the kernel: ``pmm_norms_f32_device`` for the
norms (the values the f32 path uses), an integer round-to-nearest-even in NumPy
for the image, a float64 NumPy ratio for the residual bound.

The bracket of ``rel`` on a safe row, rho <= rel <= min(rho (1 + 2^-8) + 2^-20,
2^-8): the kernel inflates its measured ratio by 2^-9; its f32 sums of at most
1500 squares and the square root are each within about 1e-4 relative (d * 2^-24
for a sequential sum), far inside the 2^-9 (1.95e-3) on the low side and the
2^-8 - 2^-9 left on the high side.  tests/test_screen_corpus_cpu.py evaluates
the formula in f32 NumPy on these very draws and checks the same bracket.
"""
from __future__ import annotations

import numpy as np
import pytest

from polars_matmul import _native

pytestmark = pytest.mark.gpu

ROWS = 70
DIMS = [1, 3, 8, 37, 128, 255, 256, 257, 700, 768, 1500]
FIRST_SAFE = 20  # rows [FIRST_SAFE, ROWS) are plain draws: all safe
CAP = np.float32(2.0 ** -8)

# bf16 halfway cases of both parities (down to the even 0x3F80, up to the even
# 0x3F82), signed zeros, denormals, a value that rounds up to inf, infinities
HALF_DOWN, HALF_UP = np.array([0x3F808000, 0x3F818000], dtype=np.uint32).view(np.float32)
# (row, value): one special per row, at column (7 * row) % d
PLANTED = [(0, HALF_DOWN), (1, HALF_UP), (2, np.float32(-0.0)), (3, np.float32(0.0)),
           (4, np.float32(1e-40)), (5, np.float32(-1e-42)), (6, np.float32(3.4e38)), (7, np.float32(np.inf)),
           (8, np.float32(-np.inf)), (9, np.float32(np.nan)),
           # the five unsafe kinds by name (10: the zero row, below) and a row of norm 5e-7
           (11, np.float32(np.nan)), (12, np.float32(np.inf)), (13, np.float32(1e-40)),
           (14, np.float32(2.0 ** 49))]
ZERO_ROW, TINY_NORM_ROW = 10, 15
UNSAFE_ROWS = {4, 5, 6, 7, 8, 9, ZERO_ROW, 11, 12, 13, 14, TINY_NORM_ROW}


def draw(d, seed=0):
    """randn scaled per row by a power of two inside the window, with the specials planted."""
    rs = np.random.RandomState(1000 * d + seed)
    a = (rs.randn(ROWS, d) * np.exp2(rs.randint(-10, 21, (ROWS, 1)))).astype(np.float32)
    for r in range(FIRST_SAFE):  # unit scale: a planted finite value decides nothing but its own element
        a[r] = rs.randn(d).astype(np.float32)
    for r, v in PLANTED:
        a[r, (7 * r) % d] = v
    a[ZERO_ROW] = 0.0
    a[TINY_NORM_ROW] = 0.0
    a[TINY_NORM_ROW, (7 * TINY_NORM_ROW) % d] = np.float32(5e-7)  # inside the window, norm below 1e-6
    bad = unsafe_rule(a)
    # the named kinds are all there; at d = 1 the planted zeros make zero rows of rows 2 and 3
    assert set(np.nonzero(bad)[0]) == (UNSAFE_ROWS | {2, 3} if d == 1 else UNSAFE_ROWS)
    return a, bad


def unsafe_rule(a):
    """The unsafe flag by its definition: a non-finite element, a non-zero one outside [2^-48, 2^48], a norm
    at or below 1e-6, a zero sum.  (No row of these draws has a norm near 1e-6, where f32 would decide.)"""
    ax = np.abs(a.astype(np.float64))
    with np.errstate(all="ignore"):
        window = np.isfinite(ax) & ((ax == 0) | ((ax >= 2.0 ** -48) & (ax <= 2.0 ** 48)))
        norm = np.sqrt((np.where(np.isfinite(ax), ax, 0.0) ** 2).sum(axis=1))
    assert not (np.abs(norm - 1e-6) < 1e-8).any()
    return (~window.all(axis=1) | ~(norm > 1e-6)).astype(np.uint32)


def rne_bits(a):
    """bf16 bit patterns of f32 values, round to nearest even in integers (not for NaN)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def is_nan_bf16(b):
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def rho64(a):
    """||x - bf16(x)|| / ||x|| per row in float64 (rows of finite values)."""
    x = a.astype(np.float64)
    xb = (rne_bits(a).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt(((x - xb) ** 2).sum(axis=1) / (x ** 2).sum(axis=1))


def run(a, d, aligned, scal=True, skip=()):
    """The kernel over a's rows placed at an aligned (16-byte base, stride a multiple of 4) or a
    misaligned (base off by one float, odd stride) source.  Returns the outputs and the norms reference."""
    import torch

    dev = torch.device("cuda:0")
    rows = a.shape[0]
    ld = -(-d // 4) * 4 if aligned else (d + 5 if (d + 5) % 2 else d + 6)
    off = 0 if aligned else 1
    host = np.full(rows * ld + 1, 777.0, dtype=np.float32)  # (what lies between the rows is not part of them)
    host[off:off + rows * ld].reshape(rows, ld)[:, :d] = a
    src = torch.from_numpy(host).to(dev)
    ptr = src.data_ptr() + 4 * off
    assert (ptr % 16 == 0 and ld % 4 == 0) == aligned
    ldo = -(-d // 128) * 128
    out = torch.full((rows, ldo), -1, dtype=torch.int16, device=dev)  # 0xFFFF: unwritten padding shows
    f = {k: torch.full((rows,), 12345.0, dtype=torch.float32, device=dev) for k in ("norm", "inv_norm", "rel")}
    bad = torch.full((rows,), 99, dtype=torch.int32, device=dev)
    pair = torch.zeros(2, dtype=torch.int32, device=dev)
    ref = torch.empty((rows,), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _native.screen_prepare_device(ptr, ld, rows, d, out.data_ptr(), ldo,
                                  norm=0 if "norm" in skip else f["norm"].data_ptr(),
                                  inv_norm=0 if "inv_norm" in skip else f["inv_norm"].data_ptr(),
                                  rel=0 if "rel" in skip else f["rel"].data_ptr(),
                                  unsafe=0 if "unsafe" in skip else bad.data_ptr(),
                                  scalars=pair.data_ptr() if scal else 0, stream=st)
    _native.norms_device(ptr, ld, rows, d, False, ref.data_ptr(), stream=st)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in f.items()}
    got["unsafe"] = bad.cpu().numpy()
    got["image"] = out.cpu().numpy().view(np.uint16)
    got["pair"] = pair.cpu().numpy().view(np.uint32)
    return got, ref.cpu().numpy()


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


def check(a, want_bad, d, aligned, label):
    got, rn = run(a, d, aligned)
    rows = a.shape[0]
    # exact norm and factor of the unrounded row
    assert same_bits(got["norm"], rn).all(), f"{label}: norms differ in rows {np.nonzero(~same_bits(got['norm'], rn))[0][:5]}"
    with np.errstate(all="ignore"):
        rinv = np.where(rn > np.float32(1e-6), np.float32(1.0) / rn, np.float32(0.0)).astype(np.float32)
    assert same_bits(got["inv_norm"], rinv).all(), f"{label}: factors differ"
    # the image: integer RNE, NaN stays NaN, padding zero
    img = got["image"]
    nan = np.isnan(a)
    want = rne_bits(a)
    assert np.array_equal(img[:, :d][~nan], want[~nan]), (
        f"{label}: image differs at {np.argwhere((img[:, :d] != want) & ~nan)[:4].tolist()}")
    assert is_nan_bf16(img[:, :d][nan]).all(), f"{label}: a NaN did not stay NaN"
    assert not img[:, d:].any(), f"{label}: padding columns are not zero"
    if rows == ROWS:  # the planted roundings, by value
        assert img[0, 0] == 0x3F80 and img[1, 7 % d] == 0x3F82
        assert img[2, 14 % d] == 0x8000 and img[3, 21 % d] == 0x0000
        assert img[6, 42 % d] == 0x7F80 and img[7, 49 % d] == 0x7F80 and img[8, 56 % d] == 0xFF80
    # flags
    assert np.array_equal(got["unsafe"].view(np.uint32), want_bad), (
        f"{label}: flags differ in rows {np.nonzero(got['unsafe'].view(np.uint32) != want_bad)[0].tolist()}")
    # residual bound
    safe = want_bad == 0
    rel = got["rel"]
    rho = rho64(a[safe])
    hi = np.minimum(rho * (1.0 + 2.0 ** -8) + 2.0 ** -20, 2.0 ** -8)
    assert (rel[safe].astype(np.float64) >= rho).all(), f"{label}: rel below the measured ratio"
    assert (rel[safe] <= CAP).all() and (rel[safe].astype(np.float64) <= hi).all(), (
        f"{label}: rel above its bracket: {rel[safe][rel[safe] > hi][:4]} vs {hi[rel[safe] > hi][:4]}")
    assert (rel[~safe] == CAP).all(), f"{label}: an unsafe row's rel is not 2^-8"
    # the scalar pair: maximum over the safe rows, OR of the flags
    assert got["pair"][0] == rel[safe].max().view(np.uint32), f"{label}: scalar maximum"
    assert got["pair"][1] == (1 if (~safe).any() else 0), f"{label}: scalar flag"
    return got


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("d", DIMS)
def test_screen_prepare_matches_references(d, aligned):
    assert _native.device_count() > 0, "no HIP device visible"
    a, bad = draw(d)
    check(a, bad, d, aligned, f"d={d}")
    # safe rows alone: the scalar flag stays clear
    assert not bad[FIRST_SAFE:].any()
    got = check(a[FIRST_SAFE:], bad[FIRST_SAFE:], d, aligned, f"d={d} safe rows")
    assert got["pair"][1] == 0


def test_screen_prepare_skips_null_outputs_and_the_pair():
    a, _ = draw(37)
    full, _ = run(a, 37, True)
    for skip in (("norm",), ("inv_norm", "rel"), ("unsafe",), ("norm", "inv_norm", "rel", "unsafe")):
        got, _ = run(a, 37, True, scal=False, skip=skip)
        assert np.array_equal(got["image"], full["image"])
        assert not got["pair"].any()
        for k in ("norm", "inv_norm", "rel"):
            if k in skip:
                assert (got[k] == np.float32(12345.0)).all(), f"skipped array {k} was written"
            else:
                assert same_bits(got[k], full[k]).all()
        if "unsafe" in skip:
            assert (got["unsafe"] == 99).all()
        else:
            assert np.array_equal(got["unsafe"], full["unsafe"])


def test_screen_prepare_rows_0_and_d_0_as_round_bf16():
    import torch

    dev = torch.device("cuda:0")
    src = torch.ones(8 * 4, dtype=torch.float32, device=dev)
    out = {k: torch.full((8, 8), -1, dtype=torch.int16, device=dev) for k in ("prepare", "round")}
    arr = {k: torch.full((8,), 12345.0, dtype=torch.float32, device=dev) for k in ("pn", "pi", "rel", "rn", "ri")}
    bad = torch.full((8,), 99, dtype=torch.int32, device=dev)
    # rows = 0: accepted, nothing written (null pointers included)
    _native.screen_prepare_device(0, 4, 0, 4, 0, 8)
    _native.round_bf16_device(0, 4, 0, 4, 0, 8)
    _native.screen_prepare_device(src.data_ptr(), 4, 0, 4, out["prepare"].data_ptr(), 8, norm=arr["pn"].data_ptr())
    torch.cuda.synchronize()
    assert (out["prepare"].cpu().numpy() == -1).all() and (arr["pn"].cpu().numpy() == np.float32(12345.0)).all()
    # d = 0: accepted, the rows are all padding; norm 0, factor 0 -- and no screen for such a row
    _native.screen_prepare_device(src.data_ptr(), 4, 8, 0, out["prepare"].data_ptr(), 8, norm=arr["pn"].data_ptr(),
                                  inv_norm=arr["pi"].data_ptr(), rel=arr["rel"].data_ptr(), unsafe=bad.data_ptr())
    _native.round_bf16_device(src.data_ptr(), 4, 8, 0, out["round"].data_ptr(), 8, norm=arr["rn"].data_ptr(),
                              inv_norm=arr["ri"].data_ptr())
    torch.cuda.synchronize()
    assert not out["prepare"].cpu().numpy().any() and not out["round"].cpu().numpy().any()
    for k in ("pn", "pi", "rn", "ri"):
        assert (arr[k].cpu().numpy() == 0.0).all(), k
    assert (bad.cpu().numpy() == 1).all() and (arr["rel"].cpu().numpy() == CAP).all()
    # the same argument errors
    for ld, d, ldo, off in ((16, 16, 12, 0), (16, 16, 8, 0), (8, 16, 16, 0), (16, 16, 16, 2)):
        big = torch.zeros(64 * 16, dtype=torch.float32, device=dev)
        o = torch.zeros(64 * 128, dtype=torch.int16, device=dev)
        with pytest.raises(_native.PmmError) as ei:
            _native.screen_prepare_device(big.data_ptr(), ld, 4, d, o.data_ptr() + off, ldo)
        assert ei.value.code == _native.PMM_ERR_ARG
