"""cfhip_layernorm_plan (ops.layernorm_plan), read without a GPU: the launches the last-dim LayerNorm entry points plan — kernel family,
template coordinates, grid, LDS, partial rows, workspace — as a host-side query, against a restatement of the selection rules as
csrc/norm.hip spelled them before they moved into ln_plan_fwd / ln_plan_bwd (its dispatch macros and `fused_ok`), and its refusals."""
import ctypes
import itertools

import pytest

from cflearn_amd import _lib, ops

DS = range(4, 2049, 4)
MS = (1, 2, 7, 8, 9, 4096, 4097, 100000)  # across both grid caps (512 / 1024 x 8 rows, 768 x 4 pairs) and the odd last pair
INTS = _lib.DEFINES["CFHIP_LN_PLAN_INTS"]


def _ln_grid(m, cap):
    return max(1, min(-(-m // 8), cap))


def _ln2_grid(m):
    pairs = (m + 1) // 2
    iters = -(-pairs // (768 * 4))
    return max(1, -(-pairs // (4 * iters)))


def _row(family, m, d, x32, y32, dx, pg):
    """LN_DISPATCH: 1 .. 4 chunks as they are, `case 5: case 6:` on 6 (exact only `nch == 6`), the rest on 8 (exact only `nch == 8`)"""
    nch = -(-d // 256)
    n = nch if nch <= 4 else 6 if nch <= 6 else 8
    return [family, n, int(d % 256 == 0 and nch == n), x32, y32, dx, pg, 0, _ln_grid(m, 512 if pg else 1024), 2 * d * 4 if pg else 0]


def _workspace(m, d):
    return max(_ln_grid(m, 512), _ln2_grid(m)) * 2 * d * 4


def _expect(backward, m, d, x32, y32=0, dx=0, pg=0, lo_in=0, lo_out=0, aligned=0, option=1):
    if not backward:
        launches = [_row(0, m, d, x32, y32, 0, 0)]
    else:
        nch, exact, lo = -(-d // 256), d % 256 == 0, lo_in or lo_out
        if option and (exact or option == 1) and dx and pg and d % 8 == 0 and nch <= 5 and aligned and (not lo or lo_out):  # fused_ok
            launches = [[2, min(nch, 5), int(exact), x32, 0, 1, 1, int(lo), _ln2_grid(m), (1 + 2 * 4) * nch * 256 * 4]]
        elif dx and pg and nch >= 5:  # the two recursive calls: dx alone, then the partials alone
            launches = [_row(1, m, d, x32, 0, 1, 0), _row(1, m, d, x32, 0, 0, 1)]
        else:
            launches = [_row(1, m, d, x32, 0, dx, pg)]
    flat = [v for launch in launches for v in launch]
    return [len(launches), launches[-1][8] if pg else 0, _workspace(m, d) if pg else 0] + flat + [0] * (INTS - 3 - len(flat))


def _query(lib, out, backward, m, d, x32, y32=0, dx=0, pg=0, lo_in=0, lo_out=0, aligned=0):
    flags = x32 | y32 << 1 | dx << 2 | pg << 3 | lo_in << 4 | lo_out << 5 | aligned << 6
    assert lib.cfhip_layernorm_plan(backward, m, d, flags, out) == 0, lib.cfhip_last_error()
    return list(out)


def test_forward_plan_over_the_full_grid():
    lib, out = _lib.load(), (ctypes.c_int * INTS)()
    for d, m, (x32, y32) in itertools.product(DS, MS, ((0, 0), (1, 0), (1, 1))):
        assert _query(lib, out, 0, m, d, x32, y32) == _expect(0, m, d, x32, y32), (m, d, x32, y32)


@pytest.mark.parametrize("option", (0, 1, 2))
def test_backward_plan_over_the_full_grid(option):
    lib, out = _lib.load(), (ctypes.c_int * INTS)()
    try:
        ops.set_option("ln_bwd_fused", option)
        for d, m in itertools.product(DS, MS):
            for x32, (dx, pg), lo_in, lo_out, aligned in itertools.product((0, 1), ((1, 1), (1, 0), (0, 1)), (0, 1), (0, 1), (0, 1)):
                got = _query(lib, out, 1, m, d, x32, 0, dx, pg, lo_in, lo_out, aligned)
                assert got == _expect(1, m, d, x32, 0, dx, pg, lo_in, lo_out, aligned, option), (m, d, x32, dx, pg, lo_in, lo_out, aligned)
    finally:
        ops.set_option("ln_bwd_fused", 1)


def test_workspace_size():
    """cfhip_layernorm_bwd_workspace is sized for either backward kernel, whichever the pointers' alignment selects: on every width both
    serve (D % 8 == 0, D <= 1280) it is exactly the larger `partial_rows` of the aligned16 on / off plans times 2 D 4 bytes.  On the other
    widths both plans are the row kernel's and the size query still takes the maximum over both grids, as it always has (M = 4097,
    D = 2048: 512 planned rows, 513 sized; M = 100000: 512 and 736) — there it must cover the plans and equal the old formula, which
    is also what every plan with parameter gradients reports as `workspace_bytes`, the figure the entry points check."""
    lib = _lib.load()
    for d, m in itertools.product(DS, MS):
        nbytes = lib.cfhip_layernorm_bwd_workspace(m, d)
        plans = [ops.layernorm_plan(True, m, d, want_dx=want_dx, aligned16=aligned) for want_dx in (True, False) for aligned in (True, False)]
        assert nbytes == _workspace(m, d) and all(p.workspace_bytes == nbytes for p in plans), (m, d)
        largest = max(p.partial_rows for p in plans[:2]) * 2 * d * 4
        assert nbytes >= largest and (nbytes == largest or d % 8 or d > 1280), (m, d, nbytes, largest)
        assert ops.layernorm_plan(True, m, d, want_param_grads=False).workspace_bytes == 0


def _families(plan):
    return [(l.family, l.n, l.exact, l.do_dx, l.do_pg) for l in plan.launches]


def test_plan_edges():
    m = 70
    assert _families(ops.layernorm_plan(True, m, 1280)) == [("bwd_one", 5, 1, 1, 1)]
    assert _families(ops.layernorm_plan(True, m, 1284)) == [("bwd_row", 6, 0, 1, 0), ("bwd_row", 6, 0, 0, 1)]
    # 1288 = 5 x 256 + 8: six chunks, beyond the one-launch kernel's five, and not a multiple of 256 — aligned or not, what 1284 runs
    assert _families(ops.layernorm_plan(True, m, 1288)) == [("bwd_row", 6, 0, 1, 0), ("bwd_row", 6, 0, 0, 1)]
    assert _families(ops.layernorm_plan(True, m, 1280, aligned16=False)) == [("bwd_row", 6, 0, 1, 0), ("bwd_row", 6, 0, 0, 1)]
    assert _families(ops.layernorm_plan(True, m, 1536)) == [("bwd_row", 6, 1, 1, 0), ("bwd_row", 6, 1, 0, 1)]
    assert _families(ops.layernorm_plan(True, m, 1792)) == [("bwd_row", 8, 0, 1, 0), ("bwd_row", 8, 0, 0, 1)]
    assert _families(ops.layernorm_plan(True, m, 2048)) == [("bwd_row", 8, 1, 1, 0), ("bwd_row", 8, 1, 0, 1)]
    assert _families(ops.layernorm_plan(False, m, 1792)) == [("fwd_row", 8, 0, 0, 0)] and _families(ops.layernorm_plan(False, m, 2048)) == [("fwd_row", 8, 1, 0, 0)]
    assert _families(ops.layernorm_plan(True, m, 12)) == [("bwd_row", 1, 0, 1, 1)]  # D % 8 != 0: both outputs from one row-kernel launch
    assert _families(ops.layernorm_plan(True, m, 768, lo_in=True)) == [("bwd_row", 3, 1, 1, 1)]  # no second output word: not the LO form
    one = ops.layernorm_plan(True, m, 768, lo_in=True, lo_out=True).launches
    assert _families(ops.layernorm_plan(True, m, 768, lo_out=True)) == [("bwd_one", 3, 1, 1, 1)] and one[0].family == "bwd_one" and one[0].lo == 1
    # grids, LDS, partial rows: 70 rows = 9 workgroups of 8 waves, 35 pairs = 9 workgroups of 4 waves; 100 000 rows meet the caps
    p = ops.layernorm_plan(True, m, 1284)
    assert (p.partial_rows, p.launches[0].grid, p.launches[0].lds_bytes, p.launches[1].grid, p.launches[1].lds_bytes) == (9, 9, 0, 9, 2 * 1284 * 4)
    p = ops.layernorm_plan(True, 100000, 1284)
    assert (p.partial_rows, p.launches[0].grid, p.launches[1].grid, p.workspace_bytes) == (512, 1024, 512, 736 * 2 * 1284 * 4)
    p = ops.layernorm_plan(True, 100000, 320, x_f32=True)
    assert p.launches == (ops.LnLaunch("bwd_one", 2, 0, 1, 0, 1, 1, 0, 736, 9 * 512 * 4),) and p.partial_rows == 736
    try:
        ops.set_option("ln_bwd_fused", 2)  # the one-launch kernel for multiples of 256 only
        assert _families(ops.layernorm_plan(True, m, 320)) == [("bwd_row", 2, 0, 1, 1)]
        assert _families(ops.layernorm_plan(True, m, 512)) == [("bwd_one", 2, 1, 1, 1)]
        ops.set_option("ln_bwd_fused", 0)
        assert _families(ops.layernorm_plan(True, m, 512)) == [("bwd_row", 2, 1, 1, 1)]
    finally:
        ops.set_option("ln_bwd_fused", 1)


def test_plan_refusals():
    for backward in (False, True):
        who = "layernorm_bwd" if backward else "layernorm_fwd"
        for (m, d), msg in (((70, 6), f"{who}: D=6 must be a multiple of 4 and <= 2048"), ((70, 2052), f"{who}: D=2052 must be a multiple of 4"),
                            ((0, 768), f"{who}: empty problem"), ((70, 0), f"{who}: empty problem")):
            with pytest.raises(RuntimeError, match=msg):
                ops.layernorm_plan(backward, m, d)
    with pytest.raises(RuntimeError, match="layernorm_bwd: nothing to compute"):
        ops.layernorm_plan(True, 70, 768, want_dx=False, want_param_grads=False)
    with pytest.raises(RuntimeError, match="layernorm_fwd: an f32 output is built for f32 rows only"):
        ops.layernorm_plan(False, 70, 768, y_f32=True)
    lib, out = _lib.load(), (ctypes.c_int * INTS)()
    assert lib.cfhip_layernorm_plan(1, 70, 768, 128 | 12, out) == -1 and b"layernorm_plan" in lib.cfhip_last_error()
    assert lib.cfhip_layernorm_plan(1, 70, 768, 12, None) == -1
    assert _lib.host_query("cfhip_layernorm_plan") and _lib.ctypes_only("cfhip_layernorm_plan")
