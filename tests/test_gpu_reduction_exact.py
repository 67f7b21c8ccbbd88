"""sc_wgrad and sc_tbl_sum (csrc/wgrad.hip) in exact arithmetic.

Every operand is a small dyadic number, so every fp32 product and every partial sum the kernels can form is exactly representable:
whatever the summation order (per-wave registers, LDS, per-workgroup partial images, float atomics), the result must be BIT-equal to
the float64 sum.  A dropped, duplicated or mis-imaged point, a padding lane that is summed, or a partial image added twice then fails
outright instead of hiding under a relative bar.

Exactness bounds (x: a TBL64 operand, c: a coefficient / second operand):
  tbl_sum, no coef : x = k / 64, |k| <= 32.  Every partial sum is a multiple of 2^-6 of magnitude <= 32 n  (in units of 2^-6);
                     exact while 32 n < 2^24, i.e. n < 524,288 points in one image.  Largest n here: 131,088.
  tbl_sum, coef    : c = j / 8, |j| <= 4.  Products are multiples of 2^-9 of magnitude <= 128 units;  exact while 128 n < 2^24,
                     i.e. n < 131,072.  Largest n here: 40,000.
  sc_wgrad         : A = k / 64, |k| <= 32;  B = j / 64, |j| <= 8.  Products are multiples of 2^-12 of magnitude <= 256 units;
                     exact while 256 n < 2^24, i.e. n < 65,536.  Largest n here: 40,000 (past one persistent sweep of 2048 waves x
                     16 points = 32,768).  Row sums of A: multiples of 2^-6, <= 32 n units.
  sc_wgrad, PE     : the raw-coordinate columns of the positional encoding are the point itself, x = k / 64, |k| <= 64:  products
                     <= 2048 units of 2^-12, exact while n < 8,192 (n <= 1040 here).  The sin / cos columns use the hardware sine and
                     are held to a tolerance instead."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _dyadic(shape, kmax, denom, g):
    return (torch.randint(-kmax, kmax + 1, shape, generator=g).double() / denom)


def _tbl(rows, pad=0.0):
    """[n, 64] -> TBL64 (packing.rows_to_tbl's layout) with the padding lanes of the last tile set to `pad`."""
    from shapeclipper_amd import packing
    n = rows.shape[0]
    nt = packing.n_tiles(n)
    full = torch.full((nt * 16, 64), pad, dtype=torch.float32)
    full[:n] = rows.float()
    return full.view(nt, 16, 16, 4).permute(0, 2, 1, 3).contiguous().view(-1).to(DEV)


def _bits_equal(a, b):
    """Bit-identical.  The float64 references add + 0.0: a sum the kernel starts from +0 is never -0, a one-term product may be."""
    a, b = a.detach().cpu().contiguous().float(), b.detach().cpu().contiguous().float()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _rows(x, n):
    """TBL64 on the device -> [n, 64] float64 on the host."""
    from shapeclipper_amd import packing
    return packing.tbl_to_rows(x, n).cpu().double()


def _image_of(n, n_per_image, n_images):
    return torch.clamp(torch.arange(n) // n_per_image, max=n_images - 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# tbl_sum / tbl_sum_multi
# ---------------------------------------------------------------------------------------------------------------------------------
def _tbl_sum_ref(rows_list, n_per_image, n_images, coef):
    n = rows_list[0].shape[0]
    img = _image_of(n, n_per_image, n_images)
    K = 3 if coef is not None else 1
    out = torch.zeros(len(rows_list), n_images, K, 64, dtype=torch.float64)
    for t, rows in enumerate(rows_list):
        for k in range(K):
            w = rows * (coef[:, k:k + 1] if coef is not None else 1.0)
            out[t, :, k].index_add_(0, img, w)
    return out


def _fixed_mode(n, n_per_image, n_images, n_tensors, K):
    """The mode ops.tbl_sum_multi picks (restated, so that a case can assert which one it exercises)."""
    from shapeclipper_amd import _lib
    blocks = int(_lib.load().sc_tbl_sum_blocks(ctypes.c_int(n)))
    return n_per_image % 16 == 0 and blocks * n_tensors * n_images * K * 64 <= (1 << 26)


TBL_CASES = [(1, 1), (15, 1), (15, 15), (16, 1), (16, 16), (17, 1), (17, 17), (1040, 1), (1040, 16), (1040, 1040), (1020, 17),
             (40000, 16), (40000, 1), (40000, 40000), (39984, 17)]


@pytest.mark.parametrize("with_coef", [False, True])
@pytest.mark.parametrize("n,n_per_image", TBL_CASES)
def test_tbl_sum_multi_exact(n, n_per_image, with_coef):
    """Three tensors in one launch, both reduction modes (fixed order when n_per_image % 16 == 0, float atomics otherwise)."""
    from shapeclipper_amd import ops
    n_images = max(1, n // n_per_image)
    g = torch.Generator().manual_seed(n * 31 + n_per_image)
    rows = [_dyadic((n, 64), 32, 64, g) for _ in range(3)]
    coef = _dyadic((n, 3), 4, 8, g) if with_coef else None
    K = 3 if with_coef else 1
    assert (n_per_image if n_images > 1 else n) * (128 if with_coef else 32) < (1 << 24)       # the exactness bound of the docstring
    fixed = _fixed_mode(n, n_per_image, n_images, 3, K)
    assert fixed == (n_per_image % 16 == 0)
    xs = [_tbl(r) for r in rows]
    cd = coef.float().to(DEV) if with_coef else None
    got = ops.tbl_sum_multi(xs, n, n_per_image, n_images, cd)
    torch.cuda.synchronize()
    want = _tbl_sum_ref(rows, n_per_image, n_images, coef)
    assert got.shape == want.shape
    assert _bits_equal(got, want), float((got.cpu().double() - want).abs().max())


@pytest.mark.parametrize("with_coef", [False, True])
@pytest.mark.parametrize("n,n_per_image", [(1040, 16), (40000, 16), (40000, 40000), (131072, 1024)])
def test_tbl_sum_fixed_order_repeats(n, n_per_image, with_coef):
    """The fixed-order mode on ordinary fp32 data, where the rounding depends on the order of the additions: three runs are
    bit-identical (dyadic operands could not show a lost order -- every order gives the same exact sum)."""
    from shapeclipper_amd import ops
    n_images = n // n_per_image
    K = 3 if with_coef else 1
    assert _fixed_mode(n, n_per_image, n_images, 2, K)
    g = torch.Generator().manual_seed(n + 7)
    xs = [_tbl(torch.randn(n, 64, generator=g)) for _ in range(2)]
    cd = torch.randn(n, 3, generator=g).to(DEV) if with_coef else None
    runs = [ops.tbl_sum_multi(xs, n, n_per_image, n_images, cd).clone() for _ in range(3)]
    torch.cuda.synchronize()
    want = _tbl_sum_ref([_rows(x, n) for x in xs], n_per_image, n_images, cd.cpu().double() if with_coef else None)
    assert float((runs[0].cpu().double() - want).abs().max()) > 0.0        # the data does round: the check below can bite
    assert _bits_equal(runs[0], runs[1]) and _bits_equal(runs[0], runs[2])


@pytest.mark.parametrize("n_images", [8192, 8193])
def test_tbl_sum_switches_to_atomics_at_the_partial_cap(n_images):
    """16 points per image: 8192 images need exactly 2^26 floats of partial images (fixed order), 8193 need more (atomics)."""
    from shapeclipper_amd import ops
    n = 16 * n_images
    g = torch.Generator().manual_seed(n_images)
    rows = _dyadic((n, 64), 32, 64, g)
    assert _fixed_mode(n, 16, n_images, 1, 1) == (n_images == 8192)
    x = _tbl(rows)
    got = ops.tbl_sum(x, n, 16, n_images)
    torch.cuda.synchronize()
    assert _bits_equal(got, _tbl_sum_ref([rows], 16, n_images, None)[0])


@pytest.mark.parametrize("n,n_per_image", [(17, 17), (1040, 16), (1020, 17), (74, 37)])
def test_tbl_sum_ignores_nan_padding_lanes(n, n_per_image):
    from shapeclipper_amd import ops
    n_images = n // n_per_image
    g = torch.Generator().manual_seed(n)
    rows = _dyadic((n, 64), 32, 64, g)
    coef = _dyadic((n, 3), 4, 8, g).float().to(DEV)
    for c in (None, coef):
        clean = ops.tbl_sum(_tbl(rows), n, n_per_image, n_images, c)
        dirty = ops.tbl_sum(_tbl(rows, NAN), n, n_per_image, n_images, c)
        torch.cuda.synchronize()
        assert torch.isfinite(dirty).all() and _bits_equal(dirty, clean)


# ---------------------------------------------------------------------------------------------------------------------------------
# sc_wgrad: out[a][b] = sum_p A[p][a] * B[p][b]  (partial image per workgroup, then sc_partial_reduce in a fixed order)
# ---------------------------------------------------------------------------------------------------------------------------------
def _pe_columns(pts, symmetric):
    """The 48 B columns sc_wgrad's OP_PE segment forms from a point (csrc/wgrad.hip pe_lane_setup): coordinate tile c, column j =
    step * 4 + gq; gq == 3 is the raw coordinate (step 0) or zero, otherwise sin / cos (odd step) of 2^(2 gq + step // 2) * x_c."""
    x = pts.double().clone()
    if symmetric:
        x[:, 0] = x[:, 0].abs()
    cols = []
    for c in range(3):
        for j in range(16):
            step, gq = j >> 2, j & 3
            if gq == 3:
                cols.append(x[:, c] if step == 0 else torch.zeros_like(x[:, c]))
            else:
                a = x[:, c] * float(1 << (2 * gq + (step >> 1)))
                cols.append(torch.cos(a) if step & 1 else torch.sin(a))
    return torch.stack(cols, 1)


def _run_wgrad(terms, pts, n, nb0, nb1, off, ld, rowsum=None, n_per_image=0, n_images=0):
    """One sc_wgrad launch into a NaN-filled partial buffer, reduced in order: the elements no workgroup writes stay NaN."""
    from shapeclipper_amd import _lib, ops
    lib = _lib.load()
    stride = off + 64 * ld + 5
    partial = torch.full((ops.WGRAD_PARTS * stride,), NAN, device=DEV)
    ops._wgrad(lib, terms, pts, None, None, n, True, nb0, nb1, partial, stride, off, ld, rowsum, n_per_image, n_images)
    out = ops._partial_reduce(lib, partial, ops.WGRAD_PARTS, stride, stride, torch.empty(stride, device=DEV))
    torch.cuda.synchronize()
    return out.cpu(), stride


def _region(out, off, ld, nb):
    return out[off:off + 64 * ld].view(64, ld)[:, :nb]


def _outside_is_nan(out, off, ld, nb):
    m = torch.ones(out.shape[0], dtype=torch.bool)
    m[off:off + 64 * ld].view(64, ld)[:, :nb] = False
    return bool(torch.isnan(out[m]).all())


WG_N = [1, 15, 16, 17, 1040, 40000]


@pytest.mark.parametrize("layout", ["packed", "offset"])
@pytest.mark.parametrize("n", WG_N)
def test_wgrad_plain_one_segment_exact(n, layout):
    """OP_PLAIN A x OP_PLAIN B (nb0 = 64, nb1 = 0): the dV1 / dV2 form.  layout "offset" writes the 64 x 64 block at a non-zero offset
    of a 112-wide row (out_offset / out_ld), as the SDF W1 / W2 launches do; everything else of the partial image stays unwritten."""
    from shapeclipper_amd import ops
    g = torch.Generator().manual_seed(n + 3)
    A, Bm = _dyadic((n, 64), 32, 64, g), _dyadic((n, 64), 8, 64, g)
    off, ld = (0, 64) if layout == "packed" else (1000, 112)
    out, _ = _run_wgrad([(_tbl(A), None, ops.OP_PLAIN, _tbl(Bm), ops.OP_PLAIN, None, ops.OP_NONE)], torch.zeros(n, 3, device=DEV),
                        n, 64, 0, off, ld)
    assert _bits_equal(_region(out, off, ld, 64), (A.t() @ Bm + 0.0))
    assert _outside_is_nan(out, off, ld, 64)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1040])
def test_wgrad_two_segments_pe_and_plain(n, symmetric):
    """A x [PE 48 | plain 64] (nb0 = 48, nb1 = 64, the dV0 form): the plain segment and the PE segment's raw-coordinate columns are
    exact; the sin / cos columns are held to the hardware sine's error."""
    from shapeclipper_amd import _lib, ops
    g = torch.Generator().manual_seed(n + 5)
    A, Bm = _dyadic((n, 64), 32, 64, g), _dyadic((n, 64), 8, 64, g)
    pts = _dyadic((n, 3), 64, 64, g)
    lib = _lib.load()
    stride, off, ld = 64 * 112 + 7, 3, 112
    partial = torch.full((ops.WGRAD_PARTS * stride,), NAN, device=DEV)
    ops._wgrad(lib, [(_tbl(A), None, ops.OP_PLAIN, None, ops.OP_PE, _tbl(Bm), ops.OP_PLAIN)], pts.float().to(DEV), None, None, n,
               symmetric, 48, 64, partial, stride, off, ld)
    out = ops._partial_reduce(lib, partial, ops.WGRAD_PARTS, stride, stride, torch.empty(stride, device=DEV)).cpu()
    torch.cuda.synchronize()
    reg = _region(out, off, ld, 112)
    assert _outside_is_nan(out, off, ld, 112)
    assert _bits_equal(reg[:, 48:], (A.t() @ Bm + 0.0))
    pe_want = A.t() @ _pe_columns(pts, symmetric) + 0.0
    raw = torch.tensor([16 * c + j for c in range(3) for j in (3, 7, 11, 15)])
    assert _bits_equal(reg[:, raw], pe_want[:, raw])
    tol = 1e-5 * float(A.abs().sum(0).max()) + 1e-30
    assert float((reg[:, :48].double() - pe_want).abs().max()) <= tol


@pytest.mark.parametrize("n_per_image,n_images", [(16, 1), (16, 65), (1040, 3), (16000, 2), (16, 300)])
def test_wgrad_rowsum_per_image_exact(n_per_image, n_images):
    """rowsum: the per-image sums of term 0's A operand (the bias / latent gradients), from per-wave partial images added in order."""
    from shapeclipper_amd import ops
    n = n_per_image * n_images
    g = torch.Generator().manual_seed(n + n_images)
    A, Bm = _dyadic((n, 64), 32, 64, g), _dyadic((n, 64), 8, 64, g)
    rs = torch.full((n_images, 64), NAN, device=DEV)
    out, _ = _run_wgrad([(_tbl(A), None, ops.OP_PLAIN, _tbl(Bm), ops.OP_PLAIN, None, ops.OP_NONE)], torch.zeros(n, 3, device=DEV),
                        n, 64, 0, 0, 64, rs, n_per_image, n_images)
    assert _bits_equal(_region(out, 0, 64, 64), (A.t() @ Bm + 0.0))
    want = torch.zeros(n_images, 64, dtype=torch.float64).index_add_(0, _image_of(n, n_per_image, n_images), A)
    assert _bits_equal(rs, want)


@pytest.mark.parametrize("n", [17, 1039, 40001])
def test_wgrad_ignores_nan_padding_lanes(n):
    """TBL64 operands whose padding lanes (points n .. end of the last tile) hold NaN: finite, bit-identical to zero padding."""
    from shapeclipper_amd import ops
    g = torch.Generator().manual_seed(n)
    A, Bm = _dyadic((n, 64), 32, 64, g), _dyadic((n, 64), 8, 64, g)
    z = torch.zeros(n, 3, device=DEV)
    t = lambda a, b: [(a, None, ops.OP_PLAIN, b, ops.OP_PLAIN, None, ops.OP_NONE)]
    clean, _ = _run_wgrad(t(_tbl(A), _tbl(Bm)), z, n, 64, 0, 0, 64)
    dirty, _ = _run_wgrad(t(_tbl(A, NAN), _tbl(Bm, NAN)), z, n, 64, 0, 0, 64)
    assert torch.isfinite(_region(dirty, 0, 64, 64)).all()
    assert _bits_equal(_region(dirty, 0, 64, 64), _region(clean, 0, 64, 64))
    assert _bits_equal(_region(clean, 0, 64, 64), (A.t() @ Bm + 0.0))
