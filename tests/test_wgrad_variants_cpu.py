"""The weight-gradient parity table of tests/_wgrad_variants.py is complete and means what it says.

Host-only queries (stf_wgrad_kernel_name, stf_wgrad_plan): nothing is launched.  The table names
every kernel the router returns over a sweep of geometries, every signature selects the kernel it is
filed under in both storage builds and passes stf_wgrad's argument checks, stf_wgrad_plan gives every
case the properties it is there for (ragged last chunk, several tiles per split, short last split,
grid_blocks changing the plan, ...), and the table's split counts reach every remainder of the few-split
reduce kernel and the many-split one for 1, 4 and 9 taps.  A kernel added to the router, or a planner
change that moves a case off its edge, fails here until tests/test_wgrad_variants_gpu.py, which runs
this table, has a case for it again.
"""
import ctypes
import itertools

import pytest
import torch

import _wgrad_variants as W

DTYPES = [torch.bfloat16, torch.float16]
FAKE = 1 << 32                      # a 16-byte-aligned stand-in for device pointers


def wargs(s):
    from stfunet import _lib
    d = W.fields(s)
    g = _lib.ConvGeom(d["N"], d["Hs"], d["Ws"], d["Cs"], d["xcs"], d["Hd"], d["Wd"], d["R"], d["R"], d["stride"],
                      d["pad"], 0)
    return _lib.WgradArgs(g, FAKE + 2 * d["dyoff"], d["dycs"], d["Nout"], 3 * FAKE + 2 * d["xoff"], None, 0,
                          d["grid_blocks"])


def name_of(lib, s):
    return lib.stf_wgrad_kernel_name(ctypes.byref(wargs(s))).decode()


def plan_of(lib, s):
    sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
    assert lib.stf_wgrad_plan(ctypes.byref(wargs(s)), ctypes.byref(sp), ctypes.byref(nb)) == 0
    return sp.value, nb.value


def sweep():
    """Geometries of the completeness sweep: every conv shape the models launch, and around them."""
    for R, stride, Cs, Nout, w, strided in itertools.product((1, 2, 3, 7), (1, 2), (8, 16, 32, 64, 72, 128, 136),
                                                             (8, 32, 64, 96, 128, 256), (7, 8, 15, 16, 37),
                                                             (False, True)):
        if R == 2:
            if stride == 1:
                continue
            s = W.convt(2, 9, w, Cs, Nout)          # the ConvT-shaped launch: x is the 2x larger tensor
        else:
            s = W.sig(2, 2 * w if stride == 2 else w + 1, 2 * w if stride == 2 else w, Cs, Nout, R=R, stride=stride)
        if strided:
            s = s[:4] + (s[4] + 8,) + s[5:]
        yield s


@pytest.mark.parametrize("dtype", DTYPES)
def test_table_covers_exactly_the_kernels_the_router_names(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    seen = {name_of(lib, s) for s in sweep()}
    missing, extra = sorted(seen - set(W.TABLE)), sorted(set(W.TABLE) - seen)
    assert not missing and not extra, (missing, extra)
    assert len(W.TABLE) == 11 and all(len(cs) >= 1 for cs in W.TABLE.values())
    assert all(len(s) == len(W.FIELDS) for _, s, _ in W.cases())
    assert set(W.WIDE_4GIB) <= set(W.TABLE)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_signature_selects_its_kernel(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    every = [(n, s) for n, s, _ in W.cases()] + list(W.WIDE_4GIB.items())
    bad = [(n, s, got) for n, s in every for got in [name_of(lib, s)] if got != n]
    assert not bad, bad


def test_every_signature_passes_the_launch_checks():
    """stf_wgrad's own: channel counts and strides in eights, 16-byte-aligned operands, not transposed;
    and the geometry is one a convolution has (every tap of every output pixel inside the padded source)."""
    for n, s in [(n, s) for n, s, _ in W.cases()] + list(W.WIDE_4GIB.items()):
        d = W.fields(s)
        assert all(d[k] % 8 == 0 for k in ("Cs", "xcs", "xoff", "Nout", "dycs", "dyoff")), (n, s)
        assert d["xoff"] + d["Cs"] <= d["xcs"] and d["dyoff"] + d["Nout"] <= d["dycs"], (n, s)
        a = wargs(s)
        assert a.dy % 16 == 0 and a.x % 16 == 0 and not a.g.transposed
        for src, dst in ((d["Hs"], d["Hd"]), (d["Ws"], d["Wd"])):
            assert dst >= 1 and (dst - 1) * d["stride"] - d["pad"] + d["R"] - 1 <= src - 1 + d["pad"], (n, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_port_of_the_planner_agrees_with_the_library(dtype):
    """W.plan (whose chunk the property checks below need) gives stf_wgrad_plan's split count and
    workspace size over the sweep, with and without a workgroup budget, and for every table entry."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    sigs = [s[:-1] + (gb,) for s in sweep() for gb in (0, 3, W.CUS)]
    sigs += [s for _, s, _ in W.cases()] + list(W.WIDE_4GIB.values())
    for s in sigs:
        d, p = W.fields(s), W.plan(s)
        assert plan_of(lib, s) == (p["splits"], p["splits"] * d["Nout"] * d["R"] * d["R"] * d["Cs"] * 4), s


PROPS = {"single", "many", "ragged", "multi", "short", "images", "grid", "tiles", "low", "rows", "blocks",
         "slices", "cus"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_case_has_the_properties_it_is_there_for(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    for name, s, props in W.cases():
        assert props <= PROPS, (name, s)
        d, p = W.fields(s), W.plan(s)
        splits, _ = plan_of(lib, s)
        assert splits == p["splits"], (name, s)
        generic, chunk = p["kind"] == "generic", p["chunk"]
        has = {
            "single": splits == 1,
            "many": splits > 8,
            "rows": d["Nout"] % 64 != 0,
            "blocks": d["Nout"] > 64 and d["Cs"] > 64,
            "slices": d["xoff"] > 0 or d["dyoff"] > 0,
            "cus": d["grid_blocks"] == W.CUS,
            "grid": d["grid_blocks"] > 0 and plan_of(lib, s[:-1] + (0,))[0] != splits,
        }
        if generic:
            assert (splits - 1) * chunk < p["M"] <= splits * chunk and chunk % p["bkp"] == 0
            has["ragged"] = splits >= 2 and p["M"] % chunk != 0 and p["M"] % p["bkp"] != 0
            # the generic planner does not read the workgroup budget
            assert d["grid_blocks"] == 0 and plan_of(lib, s[:-1] + (W.CUS,))[0] == splits
        else:
            per_img = p["ty"] * p["tx"]
            assert (splits - 1) * chunk < p["nt"] <= splits * chunk
            has["multi"] = chunk >= 2
            has["short"] = splits >= 2 and p["nt"] % chunk != 0
            has["images"] = p["kind"] == "3x3" and chunk > per_img and chunk % per_img != 0 and min(p["ty"], p["tx"]) > 1
            has["tiles"] = d["Hd"] % p["ph"] != 0 and d["Wd"] % p["pw"] != 0
            has["low"] = d["Hd"] < p["ph"]
        lacking = sorted(k for k in props if not has.get(k, False))
        assert not lacking, (name, s, lacking, p)
        # the properties a comment could claim by accident are listed when they hold
        unlisted = sorted(k for k in ("single", "many", "rows", "slices", "grid", "cus") if has[k] and k not in props)
        assert not unlisted, (name, s, unlisted, p)


def test_the_table_has_the_edges_every_kernel_needs():
    by = {n: [p for _, p in cs] for n, cs in W.TABLE.items()}
    any_has = lambda n, *ks: any(all(k in p for k in ks) for p in by[n])        # noqa: E731
    for n in (W.G128, W.G64, W.GEN96, W.GEN64):
        assert any_has(n, "ragged") and any_has(n, "single"), n
    assert any_has(W.G128, "many") and any_has(W.G64, "rows") and any_has(W.GEN64, "rows")
    for n in (W.F16, W.F8):
        for k in ("tiles", "low", "images", "short", "blocks", "slices", "single"):
            assert any_has(n, k), (n, k)
    assert W.sig(1, 8, 8, 128, 128) in [s for s, _ in W.TABLE[W.F8]]           # the single-tile 1 x 8 x 8
    convt = [p for n in (W.T16_2, W.T8_2, W.T16_1, W.T8_1) for p in by[n]]
    for k in ("tiles", "multi", "short", "slices", "single"):
        assert any(k in p for p in convt), k
    assert any(W.fields(s)["Hd"] % 2 for n in (W.T16_2, W.T8_2, W.T16_1, W.T8_1) for s, _ in W.TABLE[n])
    for k in ("many", "slices", "tiles"):
        assert any_has(W.C8, k), k
    assert any_has(W.C8, "multi", "short", "grid")
    # one case per fused family at the CU count, where the workgroup budget changes the plan
    for fam in ((W.C8,), (W.F16, W.F8), (W.T16_2, W.T8_2, W.T16_1, W.T8_1)):
        assert any(any_has(n, "cus", "grid") for n in fam), fam


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_counts_reach_every_path_of_the_reduce(dtype):
    """stf_wgrad_reduce: up to 8 splits the per-tap kernel (1, 4 or 9 taps), unrolled by four with a
    remainder loop -- 1, 2, 3 (remainder only), 5 (one round + 1), 8 (two rounds, none left) -- above 8
    the generic kernel."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    seen = {1: set(), 4: set(), 9: set()}
    for _, s, _ in W.cases():
        taps = W.fields(s)["R"] ** 2
        if taps in seen:
            seen[taps].add(plan_of(lib, s)[0])
    for taps, got in seen.items():
        assert {1, 2, 3, 5, 8} <= got and max(got) > 8, (taps, sorted(got))


def test_sums_stay_exact_and_only_the_4gib_cases_are_large():
    """Integer operands in [-3, 3]: every partial sum is an integer below 2^24, exact in fp32 in any order."""
    for n, s in [(n, s) for n, s, _ in W.cases()] + list(W.WIDE_4GIB.items()):
        d = W.fields(s)
        assert d["N"] * d["Hd"] * d["Wd"] * 9 < 2 ** 24, (n, s)
    for n, s, _ in W.cases():
        assert W.x_bytes(s) <= W.LIMIT and W.dy_bytes(s) <= W.LIMIT, (n, s)
    for n, s in W.WIDE_4GIB.items():
        d = W.fields(s)
        big, small = (W.dy_bytes, W.x_bytes) if n == W.C8 else (W.x_bytes, W.dy_bytes)
        assert big(s) >= 1 << 32 and small(s) <= W.LIMIT, (n, s)
        pixels, cs = (d["Hd"] * d["Wd"], d["dycs"]) if n == W.C8 else (d["Hs"] * d["Ws"], d["xcs"])
        assert (d["N"] - 1) * pixels * cs * 2 >= 1 << 32, (n, s)       # the last image starts past 2^32
