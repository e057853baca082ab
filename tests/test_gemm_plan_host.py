"""CPU: the GEMM launch policy (csrc/gemm_plan.h gemm_plan(), through the host-only hiptsdbg_gemm_plan) for 256 compute units and the
default environment.  The launcher consumes exactly this plan, so a row here is what the GPU runs: main loop, tile height, instantiation,
grid.  The rows are the launches tests/test_gpu_gemm.py and the model forwards make; they were read off the launcher as it was before the
policy became one function and agree with a kernel trace of that build (LABNOTES.md)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")
sys.path.insert(0, PKG)

V1, PP, S3, PP2, DW, Q4, PP_E4M3 = range(7)                                     # hiptsdbg_gemm_plan_t::loop
QK, RESID, GELU, HEAD, RESID_LN, RESID_XG, RESID_LS = 1, 3, 4, 5, 9, 13, 15            # GemmEpilogue
STAT_PART, SK_WS, POS, RES_SCALE, COPY16, STAT_IN, OP8, STAMPS = (1 << i for i in range(8))
FIELDS = ["loop", "mr", "interior", "stamped", "tiles_m", "tiles_n", "grid", "block", "lds_bytes", "sk_first", "sk_slices",
          "raster_gm", "raster_gn", "epi_prio", "epi_prefetch", "error"]


class Plan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int32) for f in FIELDS]


def plan(epi, M, N, K, f16=0, shared_chip=0, features=0, ld_out=0, dim=0, cus=256, q4_mask=0):
    """(status, plan as a dict)"""
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_gemm_plan
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_uint] + [ctypes.c_int] * 3 + [ctypes.c_uint, ctypes.POINTER(Plan)]
    p = Plan()
    st = f(epi, M, N, K, f16, shared_chip, features, ld_out, dim, cus, q4_mask, ctypes.byref(p))
    return st, {k: getattr(p, k) for k in FIELDS}


PP_GEOM = dict(loop=PP, block=512, lds_bytes=128 * 1024, sk_slices=1, stamped=0, error=0)
DW_GEOM = dict(loop=DW, block=256, lds_bytes=72 * 1024, sk_slices=1, interior=0, raster_gm=0, raster_gn=0, error=0)
VIT = dict(M=25088, K=768, f16=1, shared_chip=1)              # a 32-image sub-batch of ViT-B/16 at 448: 784 tokens per image
XG_VIT = dict(VIT, epi=RESID_XG, N=768, features=STAT_PART | COPY16)

TABLE = [
    # stand-alone launches of tests/test_gpu_gemm.py (EPI_RESID, the chip to themselves)
    ("bf16 persistent", dict(epi=RESID, M=70000, N=768, K=128), dict(PP_GEOM, mr=7, tiles_m=313, tiles_n=3, grid=256, raster_gm=0, raster_gn=0, interior=0)),
    ("bf16 90 tiles", dict(epi=RESID, M=11520, N=512, K=512), dict(DW_GEOM, tiles_m=45, tiles_n=4, grid=180)),
    ("bf16 ragged small", dict(epi=RESID, M=300, N=272, K=128), dict(DW_GEOM, tiles_m=2, tiles_n=3, grid=6)),
    ("bf16 one row", dict(epi=RESID, M=1, N=16, K=64), dict(PP_GEOM, mr=7, tiles_m=1, tiles_n=1, grid=1)),
    ("half one row", dict(epi=RESID, M=1, N=16, K=64, f16=1), dict(PP_GEOM, mr=6, tiles_m=1, tiles_n=1, grid=1)),
    ("half EVA02-L proj, batch 10", dict(epi=RESID, M=10250, N=1024, K=1024, f16=1), dict(PP_GEOM, mr=6, tiles_m=54, tiles_n=4, grid=216)),
    ("half 224 rows", dict(epi=RESID, M=50176, N=768, K=768, f16=1), dict(PP_GEOM, mr=7, tiles_m=224, tiles_n=3, grid=256)),
    ("half 224 rows, odd K-tiles", dict(epi=RESID, M=66000, N=1024, K=320, f16=1), dict(PP_GEOM, mr=7, tiles_m=295, tiles_n=4, grid=256)),
    ("half 20 tiles", dict(epi=RESID, M=1025, N=1024, K=1024, f16=1), dict(DW_GEOM, tiles_m=5, tiles_n=8, grid=40)),
    ("half 256 rows, general form", dict(epi=RESID, M=32768, N=512, K=128, f16=1), dict(PP_GEOM, mr=8, interior=0, tiles_m=128, tiles_n=2, grid=256)),
    # the ViT forward's launches per sub-batch
    ("ViT q|k|v", dict(VIT, epi=QK, N=2304, dim=768), dict(PP_GEOM, mr=8, tiles_m=98, tiles_n=9, grid=256, raster_gm=8, raster_gn=6)),
    ("ViT proj / fc2", XG_VIT, dict(PP_GEOM, mr=8, interior=1, tiles_m=98, tiles_n=3, grid=256, raster_gm=0, raster_gn=0)),
    ("ViT patch GEMM", dict(XG_VIT, features=STAT_PART | COPY16 | POS), dict(PP_GEOM, mr=8, interior=0, tiles_m=98, tiles_n=3, grid=256)),
    ("ViT fc1", dict(VIT, epi=GELU, N=3072), dict(PP_GEOM, mr=8, tiles_m=98, tiles_n=12, grid=256, raster_gm=8, raster_gn=6)),
    # batch-specific tile heights / loops of the ViT forward (tests/gemm_epi_ref.py sweeps every batch; tests/test_gpu_gemm_epi.py runs each arm)
    ("ViT fc1, batch 12: 224 rows", dict(epi=GELU, M=12 * 784, N=3072, K=768, f16=1, features=STAT_IN),
     dict(PP_GEOM, mr=7, tiles_m=42, tiles_n=12, grid=256, raster_gm=8, raster_gn=6)),
    ("ViT q|k|v, batch 7: 224 rows, one round", dict(epi=QK, M=7 * 784, N=2304, K=768, f16=1, features=STAT_IN, dim=768),
     dict(PP_GEOM, mr=7, tiles_m=25, tiles_n=9, grid=225, raster_gm=8, raster_gn=6)),
    ("ViT proj / fc2, batch 45: 224 rows, general form", dict(XG_VIT, M=23 * 784, features=STAT_PART | COPY16 | SK_WS),
     dict(PP_GEOM, mr=7, interior=0, tiles_m=81, tiles_n=3, grid=243)),
    ("ViT last fc2, batch 13: two per CU", dict(epi=RESID, M=13 * 784, N=768, K=3072, f16=1, features=SK_WS), dict(DW_GEOM, tiles_m=40, tiles_n=6, grid=240)),
    ("ViT last fc2, batch 14: 192 rows", dict(epi=RESID, M=14 * 784, N=768, K=3072, f16=1, features=SK_WS),
     dict(PP_GEOM, mr=6, interior=0, tiles_m=58, tiles_n=3, grid=174)),
    ("ConvNeXt-B stage 2 fc2, batch 8: two per CU", dict(epi=RESID_LS, M=8 * 784, N=512, K=2048, f16=1, features=RES_SCALE | COPY16),
     dict(DW_GEOM, tiles_m=25, tiles_n=4, grid=100)),
    ("CAFormer stage 0 residual + LayerNorm, 32 images: persistent, one column tile", dict(epi=RESID_LN, M=32 * 9216, N=128, K=256, f16=1, shared_chip=1, features=COPY16),
     dict(PP_GEOM, mr=8, interior=0, tiles_m=1152, tiles_n=1, grid=256)),
    # EVA02-L, a sub-batch of 5 images of 1025 tokens (padded to 1032 rows): never the dw loop, which has no statistics epilogue
    ("EVA02-L proj", dict(epi=RESID_XG, M=5160, N=1024, K=1024, f16=1, shared_chip=1, features=STAT_PART | COPY16),
     dict(PP_GEOM, mr=6, interior=0, tiles_m=27, tiles_n=4, grid=108)),
    ("tag head", dict(epi=HEAD, M=32, N=10861, K=1536, f16=1, shared_chip=1), dict(PP_GEOM, mr=6, tiles_m=1, tiles_n=43, grid=43, sk_first=0)),
    # the 4-wave loop where its mask bit is set: whole tiles and an even number of K-tiles only
    ("4-wave fc1", dict(VIT, epi=GELU, N=3072, q4_mask=1 << GELU), dict(loop=Q4, mr=8, tiles_m=98, tiles_n=12, grid=256, block=256, lds_bytes=128 * 1024, error=0)),
    ("4-wave mask, odd K-tiles", dict(VIT, epi=GELU, N=3072, K=192, q4_mask=1 << GELU), dict(PP_GEOM, mr=8, tiles_m=98, tiles_n=12, grid=256)),
]


@pytest.mark.parametrize("name,launch,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table_256_cus_default_environment(name, launch, want):
    switches = [k for k in os.environ if k.startswith(("HIPTS_GEMM", "HIPTS_EPI_", "HIPTS_RESID_GENERAL")) and k != "HIPTS_GEMM_Q4"]
    assert switches == [], "the table is for the default environment"
    st, got = plan(**launch)
    assert st == 0
    assert {k: got[k] for k in want} == want, got


def test_ccip_stage2_sizes_straddle_the_dw_size_rule():
    """csrc/ccip.hip folds its wide stages' LayerNorms only where gemm_dw_size() -- the rule the plan itself uses -- does not take
    the stage's residual launches: stage 2 of the CAFormer at 384 (576 tokens x 512 columns per image) is 90 tiles at batch 20 (the dw
    loop, no fold) and 144 tiles per 32-image sub-batch at batch 64 (the persistent loop with 192-row tiles, folded)."""
    st, small = plan(RESID_XG, 20 * 576, 512, 2048, f16=1, features=COPY16)
    st2, large = plan(RESID_XG, 32 * 576, 512, 2048, f16=1, shared_chip=1, features=COPY16)
    assert st == 0 and st2 == 0
    assert small["tiles_m"] * 2 == 90 and small["loop"] == DW and small["grid"] == 180
    assert (large["loop"], large["mr"], large["tiles_m"], large["tiles_n"], large["grid"]) == (PP, 6, 96, 2, 192)
    # with the statistics epilogue asked for, the same launch stays on the persistent loop: what ccip.hip has to know beforehand
    st3, stat = plan(RESID_XG, 20 * 576, 512, 2048, f16=1, features=COPY16 | STAT_PART)
    assert st3 == 0 and stat["loop"] == PP


_CHILD = r"""
import json, sys
sys.path.insert(0, %(tests)r)
import test_gemm_plan_host as t
from hiptagsearch import _lib
out = []
for launch in %(launches)r:
    st, p = t.plan(**launch)
    out.append([st, p, _lib.last_error() if st else ""])
print("PLANS", json.dumps(out))
"""


def _plans_in_child(env_extra, launches):
    """The switches are read once per process, hence the child interpreter (as tests/test_gpu_gemm.py does)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("HIPTS_GEMM")}
    env.update(env_extra)
    code = _CHILD % {"tests": os.path.dirname(os.path.abspath(__file__)), "launches": launches}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("PLANS ")][-1][6:])


def test_split_k_tail_plan():
    fc2 = dict(epi=RESID, M=25088, N=768, K=3072, f16=1, shared_chip=1, features=SK_WS)      # 294 tiles: 256 whole + 38 x 4 slices = 408 items
    small = dict(epi=RESID, M=300, N=272, K=128, f16=1, shared_chip=1, features=SK_WS)
    (st, p, _), (st2, p2, _) = _plans_in_child({"HIPTS_GEMM_SPLITK": "4"}, [fc2, small])
    assert st == 0 and (p["loop"], p["mr"], p["sk_first"], p["sk_slices"], p["grid"], p["tiles_m"], p["tiles_n"]) == (PP, 8, 256, 4, 256, 98, 3)
    assert st2 == 0 and p2["sk_slices"] == 1 and p2["sk_first"] == 0


def test_half_operands_outside_pp_and_dw_stay_an_error():
    (st, p, msg), (st2, p2, _) = _plans_in_child({"HIPTS_GEMM": "s3"}, [dict(epi=RESID, M=784, N=768, K=768, f16=1), dict(epi=RESID, M=784, N=768, K=768)])
    assert st != 0 and p["error"] == 1 and "half-precision operands are only built for the pp and dw GEMM loops" in msg
    assert st2 == 0 and (p2["loop"], p2["tiles_m"], p2["tiles_n"], p2["grid"], p2["block"], p2["lds_bytes"]) == (S3, 4, 6, 24, 256, 72 * 1024)
