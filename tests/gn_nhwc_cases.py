"""The case table of tests/test_gpu_groupnorm_nhwc.py, shared with the host-only tests/test_groupnorm_plan_host.py.

Every case names the instantiation it is meant to hit, forward and backward, as cfhip_groupnorm_nhwc_plan spells it:
(form, VW, RPT, KC) — form 0 = group form (VW dwords per access, RPT = register tier, 0 = re-read), form 1 = slice form (KC
8-channel slots per thread).  The geometry functions below restate groupnorm.hip's thread maps (gn_group_map, gn_nhwc_map,
gn_nhwc_rows) for ONE purpose: to size the error model and to place the step on the last row-lane pass.  Which kernel runs
is never taken from here: the tests ask `ops.gn_nhwc_plan` and compare."""
from collections import namedtuple

FWD_TIERS, BWD_TIERS, VWS, KCS = (48, 96, 176, 0), (48, 88, 0), (1, 2, 4), (1, 2)
ALL_FWD = {(0, vw, t, 0) for vw in VWS for t in FWD_TIERS} | {(1, 0, 0, kc) for kc in KCS}  # 12 + 2
ALL_BWD = {(0, vw, t, 0) for vw in VWS for t in BWD_TIERS} | {(1, 0, 0, kc) for kc in KCS}  # 9 + 2

# splits: 0 = group form, else the slices per sample of the slice form; off: elements the row views start into their storage
Case = namedtuple("Case", "name b c g inner splits add off fwd bwd")


def group_vw(cpg):
    d = cpg // 2
    return 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1


def group_rpp(cpg, vw):
    return 256 // (cpg // 2 // vw)


def _grp(cpg, g, n, fwd_tier, bwd_tier, *, b=1, add=True, last=1, off=0, vw=None):
    """group form, `n` rows on the busiest thread: inner = (n - 1) * row lanes + last, 0 < last < row lanes, so the last row-lane pass
    is partly empty (only `last` threads of a channel slot own an n-th row)"""
    vw = vw or group_vw(cpg)
    rpp = group_rpp(cpg, vw)
    last = min(last, rpp - 1)
    assert 0 < last < rpp
    inner = (n - 1) * rpp + last
    name = f"grp-cpg{cpg}-g{g}-vw{vw}-n{n}" + ("" if add else "-noadd") + (f"-off{off}" if off else "")
    return Case(name, b, cpg * g, g, inner, 0, add, off, (0, vw, fwd_tier, 0), (0, vw, bwd_tier, 0))


def _slc(c, g, inner, splits, kc, *, b=1, add=True, off=0):
    name = f"slc-c{c}-g{g}-i{inner}-s{splits}" + ("" if add else "-noadd") + (f"-off{off}" if off else "")
    return Case(name, b, c, g, inner, splits, add, off, (1, 0, 0, kc), (1, 0, 0, kc))


# Group form.  Rows per thread n on both sides of every tier boundary (rpt = n * VW against 48 | 96 | 176 forward, 48 | 88 backward),
# channels per group with idle threads (10, 20, 30, 40, 60, 80: 255 or 250 of 256 threads own a slot; 6, 12: 255) and without (2, 4, 8),
# the limits cpg = 254 (VW 1, 2 row lanes, 2 idle threads) and 256 (VW 4, 8 row lanes; LDS lanes[2048], chA[256] full), G = 64.
GROUP_CASES = [
    # VW 1: rpt = n
    _grp(10, 4, 48, 48, 48, b=2, last=3),
    _grp(30, 4, 49, 96, 88, last=2),
    _grp(6, 4, 88, 96, 88, b=2, last=4),
    _grp(254, 4, 89, 96, 0),
    _grp(2, 4, 96, 96, 0, last=5, add=False),
    _grp(10, 4, 97, 176, 0, b=2, last=2),
    _grp(30, 4, 176, 176, 0, last=3),
    _grp(10, 4, 177, 0, 0),            # 8977 rows: the forward re-read tier with 51 row lanes
    _grp(254, 4, 177, 0, 0),           # 353 rows, 2 row lanes
    _grp(2, 64, 2, 48, 48, last=44),   # G = 64
    # VW 2: rpt = 2 n
    _grp(20, 2, 24, 48, 48, b=2, last=2),
    _grp(60, 2, 25, 96, 88, b=2),
    _grp(12, 2, 44, 96, 88, b=2, last=3),
    _grp(4, 2, 45, 96, 0, last=4),
    _grp(20, 2, 48, 96, 0, last=5, add=False),
    _grp(60, 2, 49, 176, 0, b=2, last=2),
    _grp(12, 2, 88, 176, 0, last=3),
    _grp(20, 2, 89, 0, 0),
    # VW 4: rpt = 4 n
    _grp(40, 2, 12, 48, 48, b=2, last=3),
    _grp(80, 2, 13, 96, 88, b=2),      # the 13th row of a VW = 4 thread: the first past the 48-dword tier
    _grp(256, 2, 22, 96, 88, last=2),
    _grp(8, 2, 23, 96, 0, last=4),
    _grp(40, 2, 24, 96, 0, last=5, add=False),
    _grp(80, 2, 25, 176, 0, b=2, last=2),
    _grp(256, 2, 44, 176, 0, last=3),
    _grp(256, 2, 45, 0, 0),            # 353 rows of C = 512
    _grp(40, 2, 45, 0, 0, last=2),
    _grp(8, 64, 2, 48, 48, last=3),    # G = 64, C = 512
]

# Row views 2 and 4 elements into their storage (4- and 8-byte aligned): channel counts that get VW 4 on aligned rows run with VW 1
ALIGN_CASES = [
    _grp(40, 2, 48, 48, 48, off=2, vw=1, last=7),   # 20 dword slots, 12 row lanes (240 threads)
    _grp(256, 2, 49, 96, 88, off=4, vw=1),          # 128 slots, 2 row lanes
    _grp(80, 2, 89, 96, 0, off=2, vw=1, last=3, add=False),
]

# Slice form: C = 40 (cpg 10: groups straddle the 8-channel slots, 51 row lanes, one idle thread), 1032 (129 slots: one row lane, 127
# idle threads), 2048 (256 slots exactly: the map's two-slot branch under KC = 1), 2056 (KC = 2, thread 0 alone owns a second slot),
# 2560 (64 threads do), 4096 (all do); G = 1, an odd cpg, 64; splits = 1, a count that does not divide the rows, the rows themselves,
# and the 4096 cap.
SLICE_CASES = [
    _slc(40, 4, 160, 7, 1, b=2),
    _slc(40, 8, 103, 1, 1, add=False),       # cpg 5
    _slc(1032, 24, 13, 13, 1),               # cpg 43, one row per slice
    _slc(1032, 1, 5, 2, 1, b=2),
    _slc(2048, 64, 19, 4, 1),
    _slc(2056, 8, 11, 3, 2, b=2),            # cpg 257
    _slc(2560, 64, 9, 9, 2, add=False),
    _slc(4096, 1, 10, 3, 2),
    _slc(4096, 64, 7, 1, 2, b=2),
    _slc(8, 2, 4100, 4096, 1),               # the cap: 4096 slices of 1 or 2 rows
]

CASES = GROUP_CASES + ALIGN_CASES + SLICE_CASES
assert len({c.name for c in CASES}) == len(CASES)
COVERED_FWD = {c.fwd for c in CASES}
COVERED_BWD = {c.bwd for c in CASES}


def geometry(case):
    """(n, rpp, first): rows n on the busiest thread per launch (per slice in the slice form), row lanes, and the first row of the last
    row-lane pass (of the last slice) — the rows from there on are the ones only some row lanes reach."""
    cpg = case.c // case.g
    if case.splits == 0:
        rpp = group_rpp(cpg, case.fwd[1])
        n = -(-case.inner // rpp)
        return n, rpp, (n - 1) * rpp
    cg8 = case.c // 8
    rpp = 1 if cg8 >= 256 else 256 // cg8
    bounds = [sl * case.inner // case.splits for sl in range(case.splits + 1)]  # gn_nhwc_rows
    n = max(-(-(bounds[i + 1] - bounds[i]) // rpp) for i in range(case.splits))
    r0, cnt = bounds[-2], bounds[-1] - bounds[-2]
    return n, rpp, r0 + (cnt - 1) // rpp * rpp


def chains(case):
    """k of assert_elementwise = the longest dependent chain of f32 additions on the planned path, + 8 for the roundings of one term
    (x + add, - mean, the products, the division by the count).
      group forward:  a thread adds its n rows x 2 VW terms into one sum, then the workgroup reduction (block_sum: 6 shuffle steps + the
                      fold of 4 wave partials, counted as 16).
      group backward: per-channel accumulators (n terms), the serial fold of the rpp row lanes, thread 0's serial sums over the cpg
                      channels — on top of the forward chain, whose error the backward inherits through mean / rstd.
      slice forward:  per-channel accumulators (n terms per slice), the rpp lane fold, the cpg-long serial sum of a group's channels,
                      Chan's merge over the S slices.
      slice backward: accumulators, lane fold, the S-long merge of the slice sums, the cpg-long s1 / s2 sums — plus the forward chain.
      dadd adds the sum of the f32 dx values (accumulators, lane fold, S slice sums) to the error dx already has."""
    n, rpp, _ = geometry(case)
    cpg = case.c // case.g
    if case.splits == 0:
        kf = n * 2 * case.fwd[1] + 16 + 8
        kb = kf + n + rpp + cpg + 8
        kd = kb + n + rpp
    else:
        kf = n + rpp + cpg + case.splits + 8
        kb = kf + n + rpp + case.splits + cpg + 8
        kd = kb + n + rpp + case.splits
    return kf, kb, kd
