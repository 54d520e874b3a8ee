"""cfhip_groupnorm_nhwc_plan (ops.gn_nhwc_plan), read without a GPU: the launcher's choice of instantiation as a host-side query,
its refusals, and that every GroupNorm the UNet configurations run lands on an instantiation tests/test_gpu_groupnorm_nhwc.py covers."""
import pytest

from gn_nhwc_cases import ALL_BWD, ALL_FWD, CASES, COVERED_BWD, COVERED_FWD

from cflearn_amd import ops

# (B, H * W, C) of tests/test_host_logic.py::test_groupnorm_nhwc_form_rule, GroupNorm(32): the zoo UNet's levels at 64^2 x 8 and
# 32^2 x 8, the concatenated skip widths, one 256^2 sample, and 3 channels per group
UNET_SHAPES = [(8, 1024, 640), (8, 1024, 320), (8, 256, 2560), (8, 64, 1280), (8, 4096, 960), (8, 4096, 640), (8, 4096, 320),
               (8, 1024, 1920), (8, 1024, 1280), (8, 1024, 960), (1, 65536, 320), (8, 4096, 96)]


def test_table_covers_every_instantiation():
    assert COVERED_FWD == ALL_FWD and COVERED_BWD == ALL_BWD
    assert len(ALL_FWD) == 12 + 2 and len(ALL_BWD) == 9 + 2


@pytest.mark.parametrize("b,inner,c", UNET_SHAPES)
def test_unet_shapes_land_on_covered_instantiations(b, inner, c):
    for backward, covered in ((False, COVERED_FWD), (True, COVERED_BWD)):
        splits = ops.gn_nhwc_splits(b, inner, c, 32, backward)
        plan = ops.gn_nhwc_plan(backward, c, 32, inner, splits)
        assert plan in covered, (b, inner, c, backward, splits, plan)
        assert (plan[0] == 0) == (splits == 0)


def test_plan_of_every_table_case():
    """the table's own expectation, without a device (the GPU test asserts the same before it launches)"""
    for case in CASES:
        assert ops.gn_nhwc_plan(False, case.c, case.g, case.inner, case.splits, case.off == 0) == case.fwd, case.name
        assert ops.gn_nhwc_plan(True, case.c, case.g, case.inner, case.splits, case.off == 0) == case.bwd, case.name


def test_plan_rule_and_refusals():
    # the UNet's widest level: 80 channels per group = 40 dwords -> 16-byte accesses, 25 row lanes, 11 rows x 4 dwords per thread
    assert ops.gn_nhwc_plan(False, 2560, 32, 256, 0) == (0, 4, 48, 0)
    assert ops.gn_nhwc_plan(False, 2560, 32, 256, 0, aligned16=False) == (0, 1, 48, 0)  # 40 slots, 6 row lanes, 43 rows
    assert ops.gn_nhwc_plan(False, 2560, 32, 295, 0, aligned16=False) == (0, 1, 96, 0)  # 50 rows
    # tier edges, VW 4 (25 row lanes): 12 | 13 rows = 48 | 52 dwords, backward 22 | 23 rows = 88 | 92
    assert ops.gn_nhwc_plan(False, 160, 2, 300, 0) == (0, 4, 48, 0) and ops.gn_nhwc_plan(False, 160, 2, 301, 0) == (0, 4, 96, 0)
    assert ops.gn_nhwc_plan(True, 160, 2, 550, 0) == (0, 4, 88, 0) and ops.gn_nhwc_plan(True, 160, 2, 551, 0) == (0, 4, 0, 0)
    assert ops.gn_nhwc_plan(False, 160, 2, 1100, 0) == (0, 4, 176, 0) and ops.gn_nhwc_plan(False, 160, 2, 1101, 0) == (0, 4, 0, 0)
    # slice form: two slots per thread only beyond 256 slots
    assert ops.gn_nhwc_plan(False, 2048, 32, 64, 4) == (1, 0, 0, 1) and ops.gn_nhwc_plan(True, 2056, 8, 64, 4) == (1, 0, 0, 2)
    # the refusals of the entry points' geometry check
    for args, msg in (((96, 32, 64, 0), "even number of channels per group"), ((4104, 8, 64, 0), "at most 4096"),
                      ((1040, 2, 64, 0), "at most 256"), ((40, 4, 16, 17), "splits = 17"), ((40, 4, 5000, 4097), "splits = 4097"),
                      ((44, 4, 16, 1), "multiple of 8"), ((1040, 65, 16, 1), "<= 64"), ((40, 4, 0, 0), "empty problem")):
        with pytest.raises(RuntimeError, match=msg):
            ops.gn_nhwc_plan(False, *args)
