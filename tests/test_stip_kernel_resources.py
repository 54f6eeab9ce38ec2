"""The space-time interest point kernels (csrc/stip.hip) as the compiler allocated them, the way tests/test_kernel_resources.py
goes: the smoothing passes hide their LDS latency behind other waves, so they must keep eight waves per SIMD."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

NAMES = ("k_stip_rows<true>", "k_stip_rows<false>", "k_stip_cols", "k_stip_products", "k_stip_response", "k_stip_count", "k_stip_scan",
         "k_stip_write", "k_stip_votes_hog", "k_stip_votes_hof", "k_stip_describe")


@pytest.fixture(scope="module")
def kernels():
    import __graft_entry__ as entry
    entry.build()
    import kernel_resources
    return {r["name"]: r for r in kernel_resources.kernels()}


def test_every_stip_kernel_is_there_without_spills_or_scratch(kernels):
    for name in NAMES:
        assert name in kernels, name
        assert not kernels[name]["vgpr_spill"] and not kernels[name]["scratch"], kernels[name]


def test_the_smoothing_kernels_keep_eight_waves_per_simd(kernels):
    """512 registers per lane and SIMD over 8 waves = 64; their LDS is all dynamic (the tile), so nothing static caps it"""
    for name in NAMES[:3]:
        r = kernels[name]
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] == 0 and r["max_wg"] == 256, r
