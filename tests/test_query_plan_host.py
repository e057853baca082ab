"""CPU: the launch plans of the query path (csrc/query_plan.h search1_plan() and sim_plan(), through the host-only hiptsdbg_search1_plan
and hiptsdbg_sim_plan).  The launchers of csrc/query.hip consume exactly these plans, so a row here is what the GPU runs: grids, group
geometry, workspace layout, which kernel takes which queries.  The switches the plans depend on are explicit bits of the entries, so
the switched-off forms are rows too."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
sys.path.insert(0, PKG)

FINISH, WIDE, TILED, PARTS, DEFAULT = 1, 2, 4, 8, 15                      # knob_bits (include/hip_tagsearch_debug.h)
S1_STATE_BYTES = 256 * 8 + 256 * 4 + 16                                  # Search1State: u64 and u32 maxima slots, four debug words
WITNESS_BYTES = 32


class Search1Plan(ctypes.Structure):
    _fields_ = ([("waves", ctypes.c_int64)] +
                [(f, ctypes.c_int32) for f in ("kk", "gw", "gl", "groups", "bcap", "finish", "grid_score", "blocks2", "blocks3", "reserved")] +
                [(f, ctypes.c_uint64) for f in ("off_wmax", "off_bcnt", "off_bflag", "off_bkey", "off_bid", "off_wit", "ws_bytes", "out_bytes", "off_flag")])


class SimPlan(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_int32) for f in ("wide_passes", "wide_grid", "last_n", "last_nqb", "last_grid", "tail_q0", "tail_passes", "tail_grid",
                                               "tail_tiled", "parts_grid", "index_passes", "reserved")] + [("parts_bytes", ctypes.c_uint64)])


def _as_dict(p):
    return {f: getattr(p, f) for f, _ in p._fields_}


def search1_plan(D, k, bits=DEFAULT):
    from hiptagsearch import _lib
    f = ctypes.CDLL(_lib.LIB_PATH).hiptsdbg_search1_plan
    f.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(Search1Plan)]
    p = Search1Plan()
    assert f(D, k, bits, ctypes.byref(p)) == 0
    return _as_dict(p)


def sim_plan(D, nq, have_tiled=1, K=300, want_parts=1, bits=DEFAULT):
    from hiptagsearch import _lib
    f = ctypes.CDLL(_lib.LIB_PATH).hiptsdbg_sim_plan
    f.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(SimPlan)]
    p = SimPlan()
    assert f(have_tiled, D, K, nq, want_parts, bits, ctypes.byref(p)) == 0
    return _as_dict(p)


def wide_passes(p):
    """[(first query, queries, query blocks, grid)] of the plan's wide passes: sim_wide_pass() of csrc/query_plan.h"""
    n = p["wide_passes"]
    return [(256 * i,) + ((p["last_n"], p["last_nqb"], p["last_grid"]) if i == n - 1 else (256, 8, p["wide_grid"])) for i in range(n)]


# D, k -> kk, gw, gl, blocks2, blocks3, groups, bcap, finish
SEARCH1 = [
    (8192, 100, dict(kk=100, gw=1, gl=32, blocks2=32, blocks3=8, groups=256, bcap=128, finish=0)),
    (8192, 1024, dict(kk=1024, gw=1, gl=4, blocks2=32, blocks3=8, groups=2048, bcap=1024, finish=0)),
    (100000, 100, dict(kk=100, gw=1, gl=64, blocks2=391, blocks3=98, groups=1564, bcap=64, finish=1)),
    (262144, 100, dict(kk=100, gw=1, gl=64, blocks2=1024, blocks3=256, groups=4096, bcap=64, finish=1)),
    (262145, 100, dict(kk=100, gw=2, gl=64, blocks2=513, blocks3=257, groups=2052, bcap=64, finish=0)),
    (1000000, 100, dict(kk=100, gw=4, gl=64, blocks2=977, blocks3=977, groups=3908, bcap=64, finish=0)),
]


def _check_layout(D, p):
    """the arrays search_one carves from the workspace follow each other without overlap, aligned as its kernels read them"""
    assert p["waves"] == (D + 63) // 64 and p["grid_score"] == (D + 127) // 128
    arrays = [("off_wmax", 8 * p["groups"], 16), ("off_bcnt", 4 * p["blocks3"], 4), ("off_bflag", 4 * p["blocks3"], 4),
              ("off_bkey", 8 * p["blocks3"] * p["bcap"], 16), ("off_bid", 4 * p["blocks3"] * p["bcap"], 4)]
    end = S1_STATE_BYTES
    for name, size, align in arrays:
        assert p[name] >= end and p[name] % align == 0 and p[name] - end < 16, (name, p)
        end = p[name] + size
    assert p["off_wit"] >= end and p["off_wit"] % 32 == 0 and p["off_wit"] - end < 32, p
    witnesses = (D + 127) // 128 * 2 * WITNESS_BYTES if p["finish"] else 0
    assert p["ws_bytes"] == p["off_wit"] + witnesses, p
    # pinned results: kk float64 scores and kk int32 ids, then the completion flag on a 64-byte line of its own
    assert p["out_bytes"] == p["kk"] * 12
    assert p["off_flag"] % 64 == 0 and 0 <= p["off_flag"] - p["out_bytes"] < 64


@pytest.mark.parametrize("D,k,want", SEARCH1, ids=["D%d-k%d" % (D, k) for D, k, _ in SEARCH1])
def test_search1_plan_table(D, k, want):
    got = search1_plan(D, k)
    assert {f: got[f] for f in want} == want, got
    _check_layout(D, got)
    off = search1_plan(D, k, DEFAULT & ~FINISH)
    assert {f: off[f] for f in want} == dict(want, finish=0), off
    assert off["ws_bytes"] == off["off_wit"]
    _check_layout(D, off)
    assert {f: off[f] for f in off if f.startswith("off_")} == {f: got[f] for f in got if f.startswith("off_")}


def test_search1_plan_fewer_documents_than_k():
    p = search1_plan(9000, 1024)
    q = search1_plan(500, 1024)
    assert p["kk"] == 1024 and q["kk"] == 500 and q["out_bytes"] == 6000 and q["off_flag"] == 6016
    _check_layout(500, q)


# D, nq -> wide passes (first query, queries, query blocks, grid), tail (first query, passes, grid), parts_grid with want_parts, index_passes
SIM = [
    (100000, 32, [], (0, 1, 391), 0, 1),
    (100000, 33, [(0, 33, 2, 256)], (33, 0, 391), 256, 1),
    (100000, 256, [(0, 256, 8, 256)], (256, 0, 391), 256, 1),
    (100000, 288, [(0, 256, 8, 256)], (256, 1, 391), 0, 2),
    (100000, 300, [(0, 256, 8, 256), (256, 44, 2, 256)], (300, 0, 391), 256, 2),
    (8192, 300, [(0, 256, 8, 256), (256, 44, 2, 64)], (300, 0, 32), 0, 2),            # the two passes' grids differ: no shared parts
    (32768, 300, [(0, 256, 8, 256), (256, 44, 2, 256)], (300, 0, 128), 256, 2),
]


@pytest.mark.parametrize("D,nq,wide,tail,parts_grid,index_passes", SIM, ids=["D%d-nq%d" % (r[0], r[1]) for r in SIM])
def test_sim_plan_table(D, nq, wide, tail, parts_grid, index_passes):
    p = sim_plan(D, nq)
    assert wide_passes(p) == wide, p
    assert (p["tail_q0"], p["tail_passes"], p["tail_grid"], p["tail_tiled"]) == tail + (1,), p
    assert p["parts_grid"] == parts_grid and p["index_passes"] == index_passes == len(wide) + tail[1], p
    assert p["parts_bytes"] == (nq + 255) // 256 * 256 * 256 * 4            # reserved whenever the caller could use the parts
    # every query is in exactly one launch
    covered = [(q0, n) for q0, n, _, _ in wide] + [(tail[0] + 32 * i, min(32, nq - tail[0] - 32 * i)) for i in range(tail[1])]
    assert [q0 for q0, _ in covered] == [sum(n for _, n in covered[:i]) for i in range(len(covered))] and sum(n for _, n in covered) == nq
    # nobody to use the maxima, or the switch off: the same launches, rowmax_kernel takes the maxima
    for q in (sim_plan(D, nq, want_parts=0), sim_plan(D, nq, bits=DEFAULT & ~PARTS)):
        assert dict(p, parts_grid=0, parts_bytes=0) == q
    # no wide pass: 32 queries a launch, over the tile-major copy where it exists and is allowed
    for kw, tiled in ((dict(bits=DEFAULT & ~WIDE), 1), (dict(K=302), 1), (dict(have_tiled=0), 0), (dict(bits=DEFAULT & ~TILED), 0)):
        q = sim_plan(D, nq, **kw)
        passes = (nq + 31) // 32
        assert (q["wide_passes"], q["tail_q0"], q["tail_passes"], q["tail_grid"], q["tail_tiled"]) == (0, 0, passes, tail[2], tiled), (kw, q)
        assert q["index_passes"] == passes and q["parts_grid"] == 0 and q["parts_bytes"] == p["parts_bytes"], (kw, q)


def test_sim_plan_many_queries_keeps_no_list():
    """nq is unbounded: three full passes, then 20 queries for the 32-query kernel; 100 000 queries are 390 full passes and a last one of 160"""
    p = sim_plan(100000, 788)
    assert wide_passes(p) == [(0, 256, 8, 256), (256, 256, 8, 256), (512, 256, 8, 256)]
    assert (p["tail_q0"], p["tail_passes"], p["parts_grid"], p["index_passes"]) == (768, 1, 0, 4)
    p = sim_plan(100000, 100000)
    assert p["wide_passes"] == 391 and wide_passes(p)[-1] == (390 * 256, 160, 8, 256) and p["tail_passes"] == 0
    assert p["parts_grid"] == 256 and p["parts_bytes"] == 391 * 256 * 256 * 4 and p["index_passes"] == 391
