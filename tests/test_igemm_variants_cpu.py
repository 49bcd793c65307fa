"""The parity table of tests/_igemm_variants.py is complete: it has a launch signature for every
implicit-GEMM variant an unforced launch can select (REACHABLE of test_igemm_routes_cpu.py), every
signature selects the variant it is filed under in both storage builds, and none outside the 4 GiB
cases is large.  Host-only queries on 256 CUs (the library's count without a GPU, and the
MI355X's): nothing is launched.  A variant added to the router fails here until it has a parity case
in tests/test_igemm_variants_gpu.py, which runs this table.
"""
import ctypes

import pytest
import torch

import _igemm_variants as V
from test_igemm_routes_cpu import REACHABLE

DTYPES = [torch.bfloat16, torch.float16]


def test_table_covers_exactly_the_reachable_variants():
    missing, extra = sorted(set(REACHABLE) - set(V.TABLE)), sorted(set(V.TABLE) - set(REACHABLE))
    assert not missing and not extra, (missing, extra)
    assert all(len(sigs) >= 1 and all(len(s) == len(V.FIELDS) for s in sigs) for sigs in V.TABLE.values())
    # register-staged without SMALLC (template argument 5): selected by a source of 4 GiB or more only
    assert set(V.SRC_4GIB) == {n for n in REACHABLE
                               if n.startswith("igemm_kernel<") and n[len("igemm_kernel<"):].split(", ")[4] == "false"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_signature_selects_its_variant(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    bad = [(n, s, got) for n, sigs in V.TABLE.items() for s in sigs for got in [V.gen.query(lib, s)[0]] if got != n]
    assert not bad, bad


def test_only_the_4gib_cases_are_large():
    for name, s in V.cases():
        assert V.src_bytes(s) <= V.LIMIT and V.dst_bytes(s) <= V.LIMIT, (name, s)
    for sigs in V.SRC_4GIB.values():
        for s in sigs:
            assert V.src_bytes(s) >= 1 << 32 and (V.fields(s)["lstm"] or V.dst_bytes(s) <= V.LIMIT), s
    for _, s, _ in V.DST_4GIB:
        assert V.dst_bytes(s) >= 1 << 32 and V.src_bytes(s) <= 2 * V.LIMIT, s


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_destinations_leave_the_tile_kernels(dtype):
    """A destination (or fused BN-backward y) of 4 GiB or more never selects a kernel that stores
    through a 32-bit buffer descriptor over it; the same launch with a dense destination does select
    the family the case is named for."""
    from stfunet import _lib
    lib = _lib.load(dtype)
    i_dcs = V.FIELDS.index("dcs")
    for (label, s, want), small in zip(V.DST_4GIB, V.DST_4GIB_SMALL):
        assert V.gen.query(lib, s)[0] == want, label
        dense = s[:i_dcs] + (V.fields(s)["Nout"],) + s[i_dcs + 1:]
        assert V.gen.query(lib, dense)[0] == small, label
        assert want.startswith("igemm_dma_kernel<")
    s, ycs, want = V.BNR_Y_4GIB
    d = V.fields(s)
    fake = 1 << 32
    g = _lib.ConvGeom(d["N"], d["Hs"], d["Ws"], d["Cs"], d["scs"], d["Hd"], d["Wd"], d["R"], d["S"], d["stride"],
                      d["pad"], d["transposed"])
    a = _lib.IgemmArgs(g, fake, 2 * fake, d["Nout"], 3 * fake, d["dcs"], None, None, 0,
                       d["N"] * d["Hd"] * d["Wd"] // d["groups"], 0, None)
    names = []
    for cs in (d["Nout"], ycs):
        bnr = _lib.BnrEpi(4 * fake, cs, fake, fake, fake, fake, 1, fake)
        a.bnr = ctypes.pointer(bnr)
        names.append(lib.stf_igemm_kernel_name(ctypes.byref(a)).decode())
    assert names == [V.DST_4GIB_SMALL[2], want]
