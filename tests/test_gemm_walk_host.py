"""CPU: the tile walk of the persistent GEMM loops (csrc/gemm_loop.h tile_origin, through the host-only hiptsdbg_gemm_tile_walk, which
calls the very function the kernels call).  Work id -> tile must be a bijection, must be the order the header describes -- restated
here in numpy from its comment: the XCD deal, then column groups / row groups / row-major -- and must hand the ids that share an XCD
(equal mod 8) one contiguous run of that order, which is what the L2 reuse of the rasters rests on."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "anime-illust-image-searcher_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BN = 256

# (tiles_m, tiles_n, raster_gm, raster_gn, tile rows)
GEOMETRIES = [
    (196, 3, 0, 0, 256),
    (196, 9, 8, 6, 256),        # last column group of 3
    (196, 12, 8, 6, 256),
    (224, 9, 8, 6, 224),        # 224-row tiles
    (13, 9, 8, 0, 256),         # ragged last row group of 5
    (5, 12, 8, 0, 256),         # group larger than the matrix
    (1, 43, 8, 6, 256),         # last column group of 1
    (7, 9, 8, 6, 256),          # 63 tiles: not a multiple of 8
    (13, 9, 8, 6, 192),         # 192-row tiles
]


def walk(tiles_m, tiles_n, gm, gn, tile_rows):
    """(row tile, column tile) per work id, from the library"""
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_gemm_tile_walk
    f.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int32)] * 2
    n = tiles_m * tiles_n
    m0, n0 = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    st = f(tiles_m, tiles_n, tile_rows, gm, gn, m0.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n0.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert st == 0
    assert (m0 % tile_rows == 0).all() and (n0 % BN == 0).all()
    return m0 // tile_rows, n0 // BN


def walk_order(tiles_m, tiles_n, gm, gn):
    """The order of the header comment as a list of (row tile, column tile): column groups of gn column tiles outermost, row-major inside
    a group (gn > 0); else groups of gm row panels, column-major inside a group (gm > 0); else row-major."""
    if gn > 0:
        return [(r, c) for c0 in range(0, tiles_n, gn) for r in range(tiles_m) for c in range(c0, min(c0 + gn, tiles_n))]
    if gm > 0:
        return [(r, c) for r0 in range(0, tiles_m, gm) for c in range(tiles_n) for r in range(r0, min(r0 + gm, tiles_m))]
    return [(r, c) for r in range(tiles_m) for c in range(tiles_n)]


def xcd_position(n):
    """Position in the order per work id: ids are dealt round-robin over 8 XCDs, and XCD x takes the x-th contiguous eighth of
    0 .. n - 1 (the first n % 8 eighths one longer), its ids in ascending order."""
    share = np.array([n // 8 + (x < n % 8) for x in range(8)])
    start = np.concatenate([[0], np.cumsum(share)[:-1]])
    ids = np.arange(n)
    return start[ids % 8] + ids // 8


def check(tiles_m, tiles_n, gm, gn, tile_rows):
    n = tiles_m * tiles_n
    tm, tn = walk(tiles_m, tiles_n, gm, gn, tile_rows)
    # every tile exactly once
    assert ((tm >= 0) & (tm < tiles_m) & (tn >= 0) & (tn < tiles_n)).all()
    assert len(set(zip(tm.tolist(), tn.tolist()))) == n
    # the order of the header comment
    order = np.array(walk_order(tiles_m, tiles_n, gm, gn), np.int64).reshape(n, 2)
    want = order[xcd_position(n)]
    assert (tm == want[:, 0]).all() and (tn == want[:, 1]).all()
    # an XCD's ids, in order, cover one contiguous run of the order
    place = {tuple(t): i for i, t in enumerate(order.tolist())}
    for x in range(min(8, n)):
        pos = np.array([place[(int(tm[i]), int(tn[i]))] for i in range(x, n, 8)])
        assert (np.diff(pos) == 1).all(), (x, pos[:16])


@pytest.mark.parametrize("tiles_m,tiles_n,gm,gn,tile_rows", GEOMETRIES, ids=["%dx%d-gm%d-gn%d" % g[:4] for g in GEOMETRIES])
def test_walk_is_the_stated_order_and_a_bijection(tiles_m, tiles_n, gm, gn, tile_rows):
    check(tiles_m, tiles_n, gm, gn, tile_rows)


QK, GELU, RESID_XG = 1, 4, 13
STAT_PART, COPY16 = 1, 16


@pytest.mark.parametrize("M", [50176, 25088])
@pytest.mark.parametrize("N", [768, 2304, 3072])
def test_walk_of_the_vit_launches_plans(M, N):
    """The geometry and raster pair the launcher hands the kernel for the ViT-B/16 launches on 256 compute units."""
    from test_gemm_plan_host import plan
    launch = {768: dict(epi=RESID_XG, features=STAT_PART | COPY16), 2304: dict(epi=QK, dim=768), 3072: dict(epi=GELU)}[N]
    st, p = plan(M=M, N=N, K=768, f16=1, shared_chip=1, cus=256, **launch)
    assert st == 0 and p["tiles_n"] == N // BN and p["mr"] in (6, 7, 8)
    assert p["tiles_m"] == -(-M // (32 * p["mr"]))
    check(p["tiles_m"], p["tiles_n"], p["raster_gm"], p["raster_gn"], 32 * p["mr"])
