"""Per-volume boundary metrics on the GPU (the volume kernels of csrc/boundary.hip through the C entry
points and stfunet.predict) against the numpy brute force of tests/_boundary3d_ref.py, which
tests/test_boundary3d_cpu.py pins to scipy and to tests/golden/boundary3d.npz bit for bit.

Bounds (u = 2^-53, the unit roundoff of float64):

* ``stf_edt3d_sq`` at spacings of at most 8 significant bits (1, 0.5, 0.625, 0.75, 2.5, 3): offsets
  are below 2^12, so every product has at most 20 bits, every square 40, every sum 42: all exact,
  and the device equals the brute force bit for bit at every voxel whatever the summation order.
* ``stf_edt3d_sq`` at generic spacings: a candidate ((sx dx)^2 + (sy dy)^2) + (sz dz)^2 carries at
  most five roundings on its longest path (the product s d, its square, two additions, and the
  first addend's own two), so a computed candidate is true (1 + d) with |d| <= g5 = 5u / (1 - 5u),
  in either association order; the minimum of perturbed candidates is within the same factor of
  the true minimum.  Device a and reference b therefore satisfy |a - b| <= 2 g5 / (1 - g5) * b
  (EDT_TOL, about 10 u).  The largest observed error over this bound is printed.
* ``stf_boundary3d_metrics``: border counts equal.  At exact spacings HD is bit-equal (the maximum
  d2 is exact and sqrt is correctly rounded on both sides); HD95 within 1e-12 relative, the 2-D
  test's bound (two square roots and one interpolation in double, numpy's and the kernel's
  interpolation formulas one rounding apart); ASSD within n u relative, n = |dP| + |dT| (two fixed
  summation orders of the same exactly rounded roots).  At generic spacings the squared distances
  themselves differ by EDT_TOL, so EDT_TOL is added to each bound (a root halves it).

The kernel-level tests use the guard-byte, two-fill (0xAA, then 0x55) harness of
test_boundary_gpu.py: equal results show that every output byte is written and that two runs agree
bit for bit; the guards must keep their fill.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from _boundary3d_ref import U, fixture_cases, fixture_spacings, stack_d2, stack_metrics
from test_boundary_gpu import DEV, EINVAL, Guarded, _u8_at_offset

pytestmark = pytest.mark.gpu
CASES = fixture_cases()
G5 = 5 * U / (1 - 5 * U)
EDT_TOL = 2 * G5 / (1 - G5)
EXACT = [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75), (3.0, 0.5, 0.625)]
GENERIC = [(2.2, 0.7, 0.7), (1.3, 0.9, 0.65)]


def _rows(spacing, V):
    s = np.asarray(spacing, np.float64)
    return np.broadcast_to(np.full(3, float(s)) if s.ndim == 0 else s, (V, 3)).copy()


def _tables(depths, spacing):
    V = len(depths)
    host = torch.zeros(V + 1, dtype=torch.int32)
    host[1:] = torch.tensor(depths).cumsum(0)
    return host, host.to(DEV), torch.from_numpy(_rows(spacing, V)).to(DEV)


def _scratch(N, H, W, V, fill):
    from stfunet import _lib
    nbytes = _lib.load().stf_boundary3d_scratch_bytes(N, H, W, V)
    assert nbytes > 0 and nbytes % 8 == 0
    return Guarded(nbytes, fill)


def run_edt(sites, depths, spacing, where=None, offset=0, fill=0xAA):
    from stfunet._lib import call, stream
    N, H, W = sites.shape
    host, starts, table = _tables(depths, spacing)
    s = _u8_at_offset(sites, offset)
    w = None if where is None else _u8_at_offset(where, offset)
    d2, scratch = Guarded(N * H * W * 8, fill), _scratch(N, H, W, len(depths), fill)
    call("stf_edt3d_sq", s.data_ptr(), None if w is None else w.data_ptr(), N, H, W, starts.data_ptr(),
         host.data_ptr(), len(depths), table.data_ptr(), d2.body.data_ptr(), scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert d2.guards_intact() and scratch.guards_intact()
    return d2.body.view(torch.float64).view(N, H, W).cpu().numpy()


def check_edt(sites, depths=None, spacing=1.0, where=None, offset=0, exact=True):
    sites = np.asarray(sites, np.uint8)
    depths = [sites.shape[0]] if depths is None else depths
    first = run_edt(sites, depths, spacing, where, offset, 0xAA)
    second = run_edt(sites, depths, spacing, where, offset, 0x55)
    assert np.array_equal(first.view(np.int64), second.view(np.int64))
    ref = stack_d2(sites, depths, spacing, where)
    if exact:
        assert np.array_equal(first, ref)
        return first, 0.0
    fin = np.isfinite(ref) & (ref > 0)
    assert np.array_equal(first[~fin], ref[~fin])
    worst = float((np.abs(first[fin] - ref[fin]) / ref[fin]).max() / EDT_TOL) if fin.any() else 0.0
    print(f"spacing {spacing}: largest |device - reference| / reference = {worst:.3f} of the bound {EDT_TOL:.3e}")
    assert worst <= 1.0
    return first, worst


def run_metrics(mask, target, depths, spacing, ignore=-1, fill=0xAA, offset=0):
    from stfunet._lib import call, stream
    N, H, W = mask.shape
    V = len(depths)
    host, starts, table = _tables(depths, spacing)
    m = _u8_at_offset(mask, offset)
    t = torch.from_numpy(np.ascontiguousarray(target, dtype=np.int64)).to(DEV)
    out, counts, scratch = Guarded(V * 24, fill), Guarded(V * 16, fill), _scratch(N, H, W, V, fill)
    call("stf_boundary3d_metrics", m.data_ptr(), t.data_ptr(), N, H, W, starts.data_ptr(), host.data_ptr(), V,
         table.data_ptr(), ignore, out.body.data_ptr(), counts.body.data_ptr(), scratch.body.data_ptr(), stream())
    torch.cuda.synchronize()
    assert out.guards_intact() and counts.guards_intact() and scratch.guards_intact()
    return (out.body.view(torch.float64).view(V, 3).cpu().numpy(),
            counts.body.view(torch.int64).view(V, 2).cpu().numpy())


def assert_metrics(out, counts, ref, ref_counts, ref_max, exact=True):
    """Device results of a stack against the brute force, with the bounds of the module docstring."""
    print("device", out.tolist(), counts.tolist(), "reference", ref.tolist(), ref_counts.tolist())
    assert np.array_equal(counts, ref_counts)
    extra = 0.0 if exact else EDT_TOL
    for v in range(len(ref)):
        if ref_max[v] is None:
            assert np.isnan(out[v]).all()
            continue
        assert not np.isnan(out[v]).any()
        if exact:
            assert out[v, 0] == np.sqrt(ref_max[v]) == ref[v, 0]
        else:
            assert abs(out[v, 0] - ref[v, 0]) <= extra * ref[v, 0]
        assert abs(out[v, 1] - ref[v, 1]) <= (1e-12 + extra) * abs(ref[v, 1])
        assert abs(out[v, 2] - ref[v, 2]) <= (int(counts[v].sum()) * U + extra) * abs(ref[v, 2])


def check_metrics(mask, target, depths=None, spacing=1.0, ignore=None, exact=True, offset=0):
    mask, target = np.asarray(mask, np.uint8), np.asarray(target, np.int64)
    depths = [mask.shape[0]] if depths is None else depths
    ign = -1 if ignore is None else ignore
    out, counts = run_metrics(mask, target, depths, spacing, ign, 0xAA, offset)
    out2, counts2 = run_metrics(mask, target, depths, spacing, ign, 0x55, offset)
    assert np.array_equal(out.view(np.int64), out2.view(np.int64)) and np.array_equal(counts, counts2)
    assert_metrics(out, counts, *stack_metrics(mask, target, depths, spacing, ignore), exact=exact)
    return out, counts


def _sites(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _blob(shape, centre, radii):
    Z, Y, X = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]]
    return (sum(((A - c) / r) ** 2 for A, c, r in zip((Z, Y, X), centre, radii)) <= 1.0).astype(np.uint8)


# ---------------------------------------------------------------- the transform
SHAPES = [(3, 5, 1), (2, 6, 63), (3, 4, 64), (2, 5, 65), (3, 6, 129), (4, 1, 70), (1, 9, 66), (2, 8, 33)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_edt_exact_spacings_bit_equal(shape):
    """W below, at and above one and two 64-voxel words, H = 1, D = 1 and D = 2; sparse and dense sites."""
    for k, (density, spacing) in enumerate(zip((0.03, 0.4, 0.03), EXACT)):
        s = _sites(shape, density, 7 * sum(shape) + k)
        s[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
        check_edt(s, spacing=spacing)
        check_edt(s, spacing=spacing, where=_sites(shape, 0.5, 900 + k))


def test_edt_generic_spacings_within_the_derived_bound():
    worst = 0.0
    for k, spacing in enumerate(GENERIC + [(0.65, 1.3, 2.2)]):
        s = _sites((6, 21, 70), 0.01, 40 + k)
        s[3, 10, 35] = 1
        worst = max(worst, check_edt(s, spacing=spacing, exact=False)[1])
        worst = max(worst, check_edt(s, depths=[1, 3, 2], spacing=spacing, where=_sites(s.shape, 0.3, 50 + k),
                                     exact=False)[1])
    print(f"largest observed error over the bound: {worst:.3f}")


def test_edt_volumes_never_see_each_other_and_empty_volumes_are_inf():
    """Depths 1, 4, 2 with one site in volume 0, one in volume 1 and none in volume 2."""
    s = np.zeros((7, 9, 70), np.uint8)
    s[0, 4, 3] = s[1, 2, 60] = 1
    d2, _ = check_edt(s, depths=[1, 4, 2], spacing=[(1, 1, 1), (3, 0.5, 0.5), (1, 1, 1)])
    assert np.isinf(d2[5:]).all() and d2[0, 4, 3] == 0 and d2[4, 2, 60] == 81.0
    assert d2[1, 4, 3] == 1.0 + 28.5 ** 2                    # its own volume's site, not the one a slice away
    where = _sites(s.shape, 0.4, 3)
    d2, _ = check_edt(s, depths=[1, 4, 2], where=where)
    assert (d2[where == 0] == -1).all() and np.isinf(d2[5:][where[5:] != 0]).all()


def test_edt_one_site_in_a_corner_longest_scans():
    s = np.zeros((12, 40, 130), np.uint8)
    s[0, 0, 0] = 1
    where = np.zeros_like(s)
    where[11, 39, 129] = where[0, 0, 129] = where[11, 0, 0] = where[6, 20, 64] = 1
    d2, _ = check_edt(s, spacing=(2.5, 0.75, 0.75), where=where)
    assert d2[11, 39, 129] == (2.5 * 11) ** 2 + (0.75 * 39) ** 2 + (0.75 * 129) ** 2


def test_edt_misaligned_base_pointer():
    s = _sites((3, 7, 67), 0.05, 11)
    check_edt(s, spacing=(3, 0.5, 0.625), where=_sites(s.shape, 0.6, 12), offset=1)
    check_edt(s, depths=[2, 1], offset=3)


def test_distance_transform_3d_python_surface():
    from stfunet import distance_transform_3d
    s = _sites((5, 11, 70), 0.02, 13)
    spacing = [(2.5, 0.75, 0.75), (1, 1, 1)]
    ref = stack_d2(s, [3, 2], spacing)
    for t in (torch.from_numpy(s), torch.from_numpy(s).bool(), torch.from_numpy(s).long() * 7):
        d2 = distance_transform_3d(t.to(DEV), depths=[3, 2], spacing=spacing)
        assert d2.dtype == torch.float64 and d2.is_cuda and np.array_equal(d2.cpu().numpy(), ref)
    where = torch.from_numpy(s[::-1].copy()).bool()
    d2 = distance_transform_3d(torch.from_numpy(s).to(DEV), [3, 2], torch.tensor(spacing), where=where.to(DEV))
    assert np.array_equal(d2.cpu().numpy(), np.where(where.numpy(), ref, -1.0))
    one = distance_transform_3d(torch.from_numpy(s).to(DEV))
    assert np.array_equal(one.cpu().numpy(), stack_d2(s))
    assert tuple(distance_transform_3d(torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV)).shape) == (0, 4, 4)


# ---------------------------------------------------------------- the metrics
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_metrics_fixture_cases(c):
    """Against the brute force and against scipy's own numbers, as committed, at both spacings."""
    for k, spacing in enumerate(fixture_spacings()):
        out, counts = check_metrics(c["P"], c["T"], spacing=spacing)
        assert counts[0].tolist() == [int(c["border_p"].sum()), int(c["border_t"].sum())]
        hd, hd95, assd = c["metrics"][k]
        if math.isnan(hd):
            assert np.isnan(out).all()
        else:
            assert out[0, 0] == hd
            assert abs(out[0, 1] - hd95) <= 1e-12 * hd95 and abs(out[0, 2] - assd) <= counts[0].sum() * U * assd


def test_metrics_generic_spacings():
    for c in CASES[3:8:2]:
        for spacing in GENERIC:
            check_metrics(c["P"], c["T"], spacing=spacing, exact=False)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_metrics_seam_shapes(shape):
    P, T = _sites(shape, 0.5, sum(shape)), _sites(shape, 0.5, sum(shape) + 1)
    P[0, 0, 0] = T[-1, -1, -1] = 1
    for spacing in EXACT[:2]:
        out, counts = check_metrics(P, T, spacing=spacing)
        if shape[0] == 1:                                     # depth 1: the border is the whole mask
            assert counts[0].tolist() == [int(P.sum()), int(T.sum())]


def _touching_stack():
    """Depths 1, 4, 2 (H x W = 12 x 66); the masks touch across both volume boundaries."""
    shape = (7, 12, 66)
    T = _blob(shape, (0.5, 5, 30), (2.6, 4, 20)) | _blob(shape, (5, 6, 40), (1.6, 4, 9))
    P = _blob(shape, (1.0, 6, 34), (2.2, 3, 16)) | _blob(shape, (4.6, 5, 37), (1.2, 5, 11))
    assert all(m[0].any() and m[1].any() and m[4].any() and m[5].any() for m in (P, T))
    return P, T, [1, 4, 2]


def test_stack_of_three_volumes_equals_each_volume_alone():
    P, T, depths = _touching_stack()
    for spacing in ((1.0, 1.0, 1.0), [(2.5, 0.75, 0.75), (3, 0.5, 0.625), (1.3, 0.9, 0.65)]):
        rows = _rows(spacing, 3)
        out, counts = check_metrics(P, T, depths, rows, exact=isinstance(spacing, tuple))
        at = 0
        for v, d in enumerate(depths):
            alone, c1 = run_metrics(P[at:at + d], T[at:at + d].astype(np.int64), [d], rows[v])
            assert np.array_equal(alone.view(np.int64), out[v:v + 1].view(np.int64)) and np.array_equal(c1, counts[v:v + 1])
            at += d
        assert not np.isnan(out).any()


def test_anisotropy_moves_the_nearest_site_between_slice_and_plane():
    P, T = np.zeros((4, 5, 9), np.uint8), np.zeros((4, 5, 9), np.uint8)
    P[1, 2, 3] = 1
    T[2, 2, 3] = T[1, 2, 5] = 1                              # one slice away; two voxels away in the plane
    assert run_edt(T, [4], 1.0, where=P)[1, 2, 3] == 1.0                  # unit spacing: the neighbouring slice
    assert run_edt(T, [4], (3.0, 1.0, 1.0), where=P)[1, 2, 3] == 4.0      # sz = 3: in the plane
    check_edt(T, spacing=(3.0, 1.0, 1.0))
    P[:], T[:] = 0, 0
    P[0, 2, 3] = 1
    T[3, 2, 3] = T[0, 2, 5] = 1                              # three slices away; two voxels away in the plane
    assert run_edt(T, [4], 1.0, where=P)[0, 2, 3] == 4.0                  # unit spacing: in the plane
    assert run_edt(T, [4], (0.5, 1.0, 1.0), where=P)[0, 2, 3] == 2.25     # sz = 0.5: three slices away
    check_edt(T, spacing=(0.5, 1.0, 1.0))
    # two identical volumes with different spacings in one table
    out, _ = check_metrics(np.concatenate([P, P]), np.concatenate([T, T]), [4, 4], [(1.0, 1.0, 1.0), (0.5, 1.0, 1.0)])
    assert out[0, 0] == 3.0 and out[1, 0] == 2.0             # T -> P: (3, 0, 0) at unit; (0, 0, 2) at sz = 0.5


def test_degenerate_volumes_in_a_stack():
    """Empty P, empty T, both, and P == T between defined neighbours."""
    g = _blob((2, 9, 70), (0.5, 4, 30), (1.5, 3, 12))
    h = _blob((2, 9, 70), (0.8, 5, 36), (1.5, 3, 9))
    e = np.zeros_like(g)
    P = np.concatenate([g, e, g, e, g, h])
    T = np.concatenate([h, g, e, e, g, g])
    out, counts = check_metrics(P, T, [2] * 6, (2.5, 0.75, 0.75))
    assert np.isnan(out[1:4]).all() and (out[4] == 0).all() and not np.isnan(out[[0, 5]]).any()
    assert counts[1, 0] == 0 and counts[2, 1] == 0 and counts[3].tolist() == [0, 0]
    assert np.array_equal(out[0, [0, 1]], out[5, [0, 1]])     # hd and hd95 are symmetric in P and T


def test_one_voxel_each_at_opposite_corners():
    P, T = np.zeros((12, 40, 130), np.uint8), np.zeros((12, 40, 130), np.uint8)
    P[0, 0, 0] = T[11, 39, 129] = 1
    out, counts = check_metrics(P, T, spacing=(2.5, 0.75, 0.75))
    d = math.sqrt((2.5 * 11) ** 2 + (0.75 * 39) ** 2 + (0.75 * 129) ** 2)
    assert out[0].tolist() == [d, d, d] and counts[0].tolist() == [1, 1]


def test_percentile_ranks_straddle_a_tie_run():
    """|dP| = |dT| = 20 single voxels on a line (D = 1), P = T except two voxels moved out by 3 and
    5: 36 zeros, then 3, 3, 5, 5; r = 0.95 * 39 = 37.05, so lo is the last 3 and hi the first 5; and
    with one of them back in place (38 zeros... 3, 3 at ranks 38, 39; lo = 37 is a zero, hi = 38 a 3)."""
    P, T = np.zeros((1, 3, 200), np.uint8), np.zeros((1, 3, 200), np.uint8)
    xs = np.arange(20) * 10
    T[0, 1, xs] = 1
    P[0, 1, xs] = 1
    P[0, 1, 0], P[0, 1, 3] = 0, 1                             # x = 0 -> 3: distances 3 both ways
    P[0, 1, 190], P[0, 1, 195] = 0, 1                         # x = 190 -> 195: 5 both ways
    out, _ = check_metrics(P, T)
    assert out[0, 0] == 5.0 and abs(out[0, 1] - (3.0 + 2.0 * 0.05)) < 1e-12
    P[0, 1, 190], P[0, 1, 195] = 1, 0
    out, _ = check_metrics(P, T, spacing=(1.0, 1.0, 0.5))
    assert out[0, 0] == 1.5 and abs(out[0, 1] - 1.5 * 0.05) < 1e-12


def test_ignore_index_and_a_mask_at_an_odd_byte_offset():
    P = _sites((3, 20, 90), 0.5, 22)
    T = _sites((3, 20, 90), 0.5, 23).astype(np.int64)
    T[:, :, 70:] = 255
    T[2, 15:, :] = 255
    out, _ = check_metrics(P, T, ignore=255, spacing=(3, 0.5, 0.625), offset=1)
    keep = T != 255
    cleared, _ = check_metrics(P * keep, T * keep, spacing=(3, 0.5, 0.625))
    assert np.array_equal(out, cleared)
    plain, _ = check_metrics(P, T, spacing=(3, 0.5, 0.625), offset=3)    # without ignore a 255 pad is foreground
    assert not np.array_equal(plain, out)


def test_boundary_metrics_3d_python_surface():
    from stfunet import boundary_metrics_3d
    P, T, depths = _touching_stack()
    T = T.astype(np.int64)
    T[3, :, 60:] = 255
    spacing = [(2.5, 0.75, 0.75), (1, 1, 1), (3, 0.5, 0.625)]
    for ignore in (None, 255):
        ref = stack_metrics(P, T, depths, spacing, ignore)
        for mask in (torch.from_numpy(P), torch.from_numpy(P).bool(), torch.from_numpy(P).int() * 3):
            for sp in (spacing, torch.tensor(spacing), torch.tensor(spacing, device=DEV, dtype=torch.float32)):
                res = boundary_metrics_3d(mask.to(DEV), torch.from_numpy(T).int().to(DEV), depths, sp, ignore)
                assert set(res) == {"hd", "hd95", "assd", "border_counts"}
                assert all(res[k].is_cuda and res[k].dtype == torch.float64 and tuple(res[k].shape) == (3,)
                           for k in ("hd", "hd95", "assd"))
                assert res["border_counts"].dtype == torch.int64 and tuple(res["border_counts"].shape) == (3, 2)
                out = torch.stack([res["hd"], res["hd95"], res["assd"]], 1).cpu().numpy()
                assert_metrics(out, res["border_counts"].cpu().numpy(), *ref)
    m, t = torch.from_numpy(P).to(DEV), torch.from_numpy(T).to(DEV)
    iso, tri = boundary_metrics_3d(m, t, spacing=0.5), boundary_metrics_3d(m, t, spacing=(0.5, 0.5, 0.5))
    unit = boundary_metrics_3d(m, t)
    for k in ("hd", "hd95", "assd"):
        assert torch.equal(iso[k], tri[k]) and torch.equal(iso[k], unit[k] * 0.5)     # a power of two scales exactly
    empty = boundary_metrics_3d(torch.zeros(0, 5, 5, dtype=torch.uint8, device=DEV),
                                torch.zeros(0, 5, 5, dtype=torch.int64, device=DEV))
    assert tuple(empty["hd"].shape) == (0,) and tuple(empty["border_counts"].shape) == (0, 2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_einval_without_a_launch(dtype):
    """Refusals with real device buffers far smaller than the refused sizes: nothing may touch them."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    buf = Guarded(8192, 0xAA)
    p = ctypes.c_void_p(buf.body.data_ptr())
    st = ctypes.c_void_p(_lib.stream())
    good = (ctypes.c_int32 * 3)(0, 1, 2)

    def bm(mask=p, target=p, N=2, H=4, W=4, sd=p, sh=good, V=2, sp=p, out=p, counts=p, scratch=p):
        return lib.stf_boundary3d_metrics(mask, target, N, H, W, sd, sh, V, sp, -1, out, counts, scratch, st)

    def edt(sites=p, N=2, H=4, W=4, sd=p, sh=good, V=2, sp=p, d2=p, scratch=p):
        return lib.stf_edt3d_sq(sites, None, N, H, W, sd, sh, V, sp, d2, scratch, st)

    for kw in ("mask", "target", "sd", "sh", "sp", "out", "counts", "scratch"):
        assert bm(**{kw: None}) == EINVAL, kw
    for kw in ("sites", "sd", "sh", "sp", "d2", "scratch"):
        assert edt(**{kw: None}) == EINVAL, kw
    odd = ctypes.c_void_p(buf.body.data_ptr() + 4)
    assert bm(out=odd) == EINVAL and bm(counts=odd) == EINVAL and bm(sp=odd) == EINVAL and edt(d2=odd) == EINVAL
    for f in (bm, edt):
        for bad in ((1, 1, 2), (0, 2, 2), (0, 0, 2), (0, 1, 3), (0, 2, 1)):
            assert f(sh=(ctypes.c_int32 * 3)(*bad)) == EINVAL, bad
        assert f(N=0) == EINVAL and f(H=0) == EINVAL and f(W=0) == EINVAL and f(V=0) == EINVAL and f(V=3) == EINVAL
        assert f(H=4097) == EINVAL and f(W=4097) == EINVAL
        assert f(N=128, H=4096, W=4096) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf.raw == 0xAA).all())


# ---------------------------------------------------------------- the predict loop
def _unet_and_loader():
    from oracle.cases import dce_case
    from oracle.init import canonical_state_dict
    from stfunet.unet import UNet
    model = UNet(in_channels=8, num_classes=2, base_c=8)
    model.load_state_dict(canonical_state_dict(model.state_dict(), seed=0))
    loader = [dce_case(500 + i, 3, 8, 32, 32) for i in range(3)]      # 9 slices in batches of 3
    return model.to(DEV), loader


@pytest.mark.parametrize("keep_largest", [False, True])
def test_predict_volumes_with_boundary_metrics(keep_largest):
    from stfunet import boundary_metrics_3d
    from stfunet.predict import predict_volumes
    model, loader = _unet_and_loader()
    depths = [2, 5, 2]                                      # both boundaries fall inside a batch
    spacing = [(2.5, 0.75, 0.75), (3.0, 0.5, 0.625), (1.0, 1.0, 1.0)]
    dev = torch.device(DEV)
    plain = predict_volumes(model, loader, dev, depths, keep_largest=keep_largest, keep_masks=True)
    again = predict_volumes(model, loader, dev, depths, keep_largest=keep_largest, keep_masks=True, boundary=False,
                            spacing=spacing)
    base = {"num", "num_volumes", "dice", "iou", "mean_dice", "mean_iou", "masks"} | (
        {"num_components"} if keep_largest else set())
    assert set(plain) == set(again) == base
    res = predict_volumes(model, loader, dev, depths, keep_largest=keep_largest, keep_masks=True, boundary=True,
                          spacing=spacing)
    assert set(res) == base | {"hd", "hd95", "assd", "mean_hd", "mean_hd95", "mean_assd", "num_boundary"}
    assert torch.equal(res["dice"], plain["dice"]) and all(torch.equal(a, b) for a, b in zip(res["masks"], plain["masks"]))
    T = torch.cat([t for _, t in loader]).to(DEV)
    direct = boundary_metrics_3d(torch.cat(res["masks"]), T, depths, spacing)
    for k in ("hd", "hd95", "assd"):
        v = res[k]
        assert v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (3,)
        assert torch.equal(v.nan_to_num(-1), direct[k].nan_to_num(-1))
        assert torch.equal(res["mean_" + k].nan_to_num(-1), torch.nanmean(direct[k]).nan_to_num(-1))
    assert res["num_boundary"].item() == int((~torch.isnan(direct["hd"])).sum()) >= 1
    ref = stack_metrics(torch.cat(res["masks"]).cpu().numpy(), T.cpu().numpy(), depths, spacing)
    got = torch.stack([res["hd"], res["hd95"], res["assd"]], 1).cpu().numpy()
    assert_metrics(got, direct["border_counts"].cpu().numpy(), *ref)
    bare = predict_volumes(model, [x for x, _ in loader], dev, depths, boundary=True)
    assert bare["hd"] is None and bare["mean_hd"] is None and bare["num_boundary"] is None
