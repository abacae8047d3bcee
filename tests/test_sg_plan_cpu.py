"""CPU-side check of the Sinkhorn plan (sg::sinkhorn_plan through rspl_sg_debug_sinkhorn_plan): which kernel, on how
many workgroups per pair and with which exchange buffers a handle of (max_keypoints, max_batch) gets on 256 CUs,
under the RSPL_SG_SINK / RSPL_SG_SINK_G overrides.  The rows restate what rspl_sg_create decided before the plan
existed (one place instead of create + run_sinkhorn + the launcher), including the order of its fall-backs."""
import ctypes as C
import re
import pathlib

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CUS = 256

# (max_keypoints, max_batch, RSPL_SG_SINK, RSPL_SG_SINK_G) -> (kind, rows per wave, workgroups per pair) or None
ROWS = [
    ((64, 1, None, None), ("sc", 4, 8)),
    ((64, 1, "sc", 4), ("sc", 8, 4)),
    ((64, 1, "sc", 16), ("sc", 2, 16)),
    ((64, 1, "sc", 32), ("sc", 1, 32)),
    ((64, 1, "slab", None), ("slab", 0, 8)),
    ((64, 1, "slab", 7), ("slab", 0, 7)),
    ((400, 1, "slab", None), ("slab", 0, 45)),
    ((240, 1, "slab", 2), ("slab_scratch", 0, 2)),
    ((400, 1, None, None), ("sc", 4, 8)),
    ((400, 2, None, None), ("sc", 4, 8)),
    ((400, 64, None, None), ("sc", 8, 4)),
    ((447, 1, None, None), ("sc", 4, 8)),
    ((448, 1, None, None), ("sc10", 3, 10)),
    ((600, 1, None, None), ("sc10", 3, 13)),
    ((600, 1, None, 16), ("sc10", 3, 16)),
    ((639, 1, None, None), ("sc10", 3, 14)),
    ((640, 1, None, None), ("wide", 4, 21)),
    ((2048, 1, None, None), ("wide", 4, 65)),
    ((2111, 1, None, None), ("wide", 4, 66)),
    ((2112, 1, None, None), ("slab_scratch", 0, 256)),
    ((4096, 1, None, None), ("slab_scratch", 0, 256)),
    ((400, 128, None, None), ("slab_scratch", 0, 2)),
    ((600, 32, None, None), ("slab_scratch", 0, 8)),
    ((2048, 4, None, None), ("slab_scratch", 0, 64)),
    ((400, 300, None, None), None),
]


def _env(monkeypatch, kind, G):
    for name, v in (("RSPL_SG_SINK", kind), ("RSPL_SG_SINK_G", G)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def test_header_and_binding():
    from rspl_slam_amd import capi
    hdr = (ROOT / "include" / "rspl.h").read_text()
    assert re.search(r"\brspl_sg_debug_sinkhorn_plan\s*\(", hdr) and re.search(r"}\s*rspl_sg_sinkhorn_plan;", hdr)
    assert "#define RSPL_ABI_VERSION 2" in hdr  # no existing struct changed
    lib = capi.load()
    assert "rspl_sg_debug_sinkhorn_plan" in capi.EXPORTS and hasattr(lib, "rspl_sg_debug_sinkhorn_plan")
    assert C.sizeof(capi.SgSinkhornPlan) == 32


@pytest.mark.parametrize("case,want", ROWS, ids=lambda v: "-".join(map(str, v)) if v and len(v) == 4 else None)
def test_plan_row(monkeypatch, case, want):
    from rspl_slam_amd import api, capi
    nmax, B, kind, G = case
    _env(monkeypatch, kind, G)
    pl = api.sinkhorn_plan(nmax, B, CUS)
    if want is None:
        assert pl is None
        pl_c = capi.SgSinkhornPlan()
        assert capi.load().rspl_sg_debug_sinkhorn_plan(nmax, B, CUS, C.byref(pl_c)) == -1  # RSPL_E_ARG
        msg = capi.load().rspl_last_error().decode()
        assert msg == f"max_batch ({B}) exceeds the CU count ({CUS}): the Sinkhorn workgroups must be co-resident"
        return
    assert (pl["kind"], pl["rows_per_wave"], pl["groups"]) == want
    assert B * pl["groups"] <= CUS  # co-resident


@pytest.mark.parametrize("nmax,kind,ug,vg", [(64, None, 1040, 65), (64, "slab", 65, 65), (600, None, 15626, 601),
                                             (2048, None, 270400, 4160)])
def test_plan_exchange_buffers(monkeypatch, nmax, kind, ug, vg):
    from rspl_slam_amd import api
    _env(monkeypatch, kind, None)
    pl = api.sinkhorn_plan(nmax, 1, CUS)
    assert (pl["ug_granules"], pl["vg_granules"]) == (ug, vg)
    # the buffers are per handle: max_batch pairs
    pl3 = api.sinkhorn_plan(nmax, 3, CUS)
    assert pl3["kind"] == pl["kind"] and (pl3["ug_granules"], pl3["vg_granules"]) == (3 * ug, 3 * vg)


def test_plan_rejects_bad_arguments():
    from rspl_slam_amd import capi
    lib, pl = capi.load(), capi.SgSinkhornPlan()
    assert lib.rspl_sg_debug_sinkhorn_plan(0, 1, CUS, C.byref(pl)) == -1
    assert lib.rspl_sg_debug_sinkhorn_plan(4097, 1, CUS, C.byref(pl)) == -1
    assert lib.rspl_sg_debug_sinkhorn_plan(64, 1, -1, C.byref(pl)) == -1
    assert lib.rspl_sg_debug_sinkhorn_plan(64, 1, CUS, None) == -1
