"""`functional.conv_route`: which of Conv2dFn's three code paths a geometry takes and how many output channels its kernels compute.
Pure host logic; the expectations are written out by hand from the predicates the function replaced."""
import pytest

from cflearn_amd import functional as HF

H, W = 20, 24
# (cin, cout, kh, kw, stride, pad, dil, h, w) -> (route, cp)
DEFAULT = [
    ((32, 32, 3, 3, 1, 1, 1, H, W), ("implicit", 32)),
    ((32, 40, 3, 3, 1, 1, 1, H, W), ("implicit", 40)),   # Cout % 32 != 0: still implicit forward (dX goes through GEMM + row2im)
    ((64, 3, 3, 3, 1, 1, 1, H, W), ("implicit", 32)),    # thin head: zero filters up to THIN_HEAD_PAD
    ((320, 5, 3, 3, 1, 1, 1, H, W), ("implicit", 32)),
    ((3, 8, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),        # Cin % 32 != 0
    ((40, 24, 3, 3, 1, 1, 1, H, W), ("im2row", 24)),
    ((32, 36, 3, 3, 1, 1, 1, H, W), ("im2row", 40)),     # Cout % 8 != 0 but not "few" channels: no thin head
    ((32, 16, 3, 3, 2, 1, 1, H, W), ("im2row", 16)),     # stride 2
    ((32, 32, 3, 3, 1, 2, 2, H, W), ("im2row", 32)),     # dilation 2
    ((32, 32, 3, 3, 1, 1, 2, H, W), ("im2row", 32)),
    ((40, 24, 1, 1, 1, 0, 1, H, W), ("pointwise", 24)),
    ((40, 3, 1, 1, 1, 0, 1, H, W), ("pointwise", 8)),    # Cout padded to the next multiple of 8
    ((3, 8, 1, 1, 1, 0, 1, H, W), ("im2row", 8)),        # 1x1 with Cin % 8 != 0
    ((32, 32, 1, 1, 2, 0, 1, H, W), ("im2row", 32)),     # 1x1 stride 2
    ((16, 8, 4, 4, 2, 1, 1, H, W), ("im2row", 8)),
    ((16, 3, 4, 4, 2, 1, 1, H, W), ("im2row", 8)),
    ((32, 32, 3, 3, 1, 1, 1, 65536, 4), ("im2row", 32)),  # the implicit kernel packs pixel coordinates into 16 bits
    ((32, 32, 3, 3, 1, 1, 1, 4, 65536), ("im2row", 32)),
    ((64, 3, 3, 3, 1, 1, 1, 65536, 4), ("im2row", 8)),
    ((32, 32, 3, 3, 1, 1, 1, 65535, 4), ("implicit", 32)),
]
NO_IMPLICIT = [  # IMPLICIT_CONV = False: the first six again
    ((32, 32, 3, 3, 1, 1, 1, H, W), ("im2row", 32)),
    ((32, 40, 3, 3, 1, 1, 1, H, W), ("im2row", 40)),
    ((64, 3, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),
    ((320, 5, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),
    ((3, 8, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),
    ((40, 24, 3, 3, 1, 1, 1, H, W), ("im2row", 24)),
    ((40, 24, 1, 1, 1, 0, 1, H, W), ("pointwise", 24)),  # (the switch does not touch the 1x1 route)
]
NO_THIN_HEAD = [  # THIN_HEAD_IMPLICIT = False: the two thin ones again
    ((64, 3, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),
    ((320, 5, 3, 3, 1, 1, 1, H, W), ("im2row", 8)),
    ((32, 32, 3, 3, 1, 1, 1, H, W), ("implicit", 32)),
]


@pytest.mark.parametrize("switch,table", [(None, DEFAULT), ("IMPLICIT_CONV", NO_IMPLICIT), ("THIN_HEAD_IMPLICIT", NO_THIN_HEAD)])
def test_conv_route_table(switch, table, monkeypatch):
    assert (HF.IMPLICIT_CONV, HF.THIN_HEAD_IMPLICIT, HF.THIN_HEAD_PAD) == (True, True, 32)
    if switch is not None:
        monkeypatch.setattr(HF, switch, False)  # (restored by the fixture)
    for geom, want in table:
        assert HF.conv_route(*geom) == want, geom
        assert HF._thin_head_ok(*geom) == (want == ("implicit", 32) and geom[1] % 8 != 0), geom
    assert {HF.IMPLICIT, HF.POINTWISE, HF.IM2ROW} == {"implicit", "pointwise", "im2row"}
