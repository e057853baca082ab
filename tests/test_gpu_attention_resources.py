"""GPU: what the loaded code object says of the attention kernel the forwards run (csrc/attn2.hip, the default geometry: variant 5, the
4-wave sequential body), read from the runtime's function attributes through hiptsdbg_attention2_kernel_resources -- nothing is launched and
no disassembly is searched.

The default kernel is compiled for four waves per SIMD (HIPTS_ATTN2_SEQ_WAVES = 4), which on gfx950's 512-register file means at most 128
registers per lane, and it has to get there WITHOUT spilling: a spilled register is reloaded inside the tile loop, where its latency lands on
the wave's MFMA chain (the one earlier attempt at four waves, the same source under a register cap, spilled and ran 127 instead of 83 us).
Its LDS is the two-slot K / V ring plus the fallback flag word, 32 KiB + 16 B, so that four workgroups fit a CU's 160 KiB."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

TOKENS_PAD = 832       # ViT-B/16 @448: 784 tokens; the kernel choice does not depend on it, but for variant 6 below two tiles


def _resources(f16, variant=0, tokens_pad=TOKENS_PAD):
    from hiptagsearch import _lib
    f = _lib.load().hiptsdbg_attention2_kernel_resources
    f.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3
    regs, scratch, lds = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(f(tokens_pad, f16, variant, ctypes.byref(regs), ctypes.byref(scratch), ctypes.byref(lds)))
    return regs.value, scratch.value, lds.value


@pytest.mark.parametrize("f16", [1, 0])
def test_default_attention_kernel_fits_four_waves_per_simd_without_scratch(f16):
    regs, scratch, lds = _resources(f16)
    print("default attention kernel, f16=%d: %d registers, %d B scratch, %d B static LDS" % (f16, regs, scratch, lds))
    assert scratch == 0, "the default attention kernel spills (%d bytes of scratch per lane)" % scratch
    assert 0 < regs <= 128, "%d registers: no four waves per SIMD" % regs
    assert lds == 2 * 2 * 8192 + 16


@pytest.mark.parametrize("f16", [1, 0])
def test_probe_describes_the_kernel_the_launch_picks(f16):
    """Variant 0 is variant 5 unless HIPTS_ATTN2 says otherwise (not set under the suite); one tile keeps variant 6 on variant 5's kernel;
    the two-block geometry (variant 1) is another kernel, with the three-slot rings."""
    assert _resources(f16, 0) == _resources(f16, 5)
    assert _resources(f16, 6, 64) == _resources(f16, 5, 64)
    assert _resources(f16, 1)[2] == 6 * 8192 + 16
