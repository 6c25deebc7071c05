"""The group descriptor's lane, stream and pair offset (csrc/sm_ctx.h: Group), where no other test pins them:
a group on every lane with per-lane scratch (AWS's weight bands), profiling records bracketed on side streams and
kept across the join, and NL's front descriptor on its own stream over both of its buffer sets.  Every case
compares maps (and launch counts) of two schedules of the same library exactly: a schedule only reorders work.
"""
import functools

import numpy as np
import pytest

from mystereomatching_amd import StereoBatch, _capi
from mystereomatching_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEYS = ("lbgr", "rbgr", "lgray", "rgray")


def _run(batch, md, profile=False, **cfg):
    """One sm_run of `batch` on a fresh context: (maps, profile_read() or None)."""
    n, H, W = batch["lgray"].shape
    sb = StereoBatch(md, H, W, n, device=0, **cfg)
    try:
        sb.profile(profile)
        sb.upload(*(batch[k] for k in KEYS))
        maps = sb.run(0.3)
        return maps, (sb.profile_read() if profile else None)
    finally:
        sb.close()


def test_aws_on_every_lane():
    """Four groups of one pair on lanes 0..3, each with its own weight band: the maps of one stream."""
    batch = S.make_batch(4, 12, 20, 8, first_index=900)
    aws = dict(aggregation="AWS", aws_radius_v=2, aws_radius_u=2)
    want, _ = _run(batch, 7, num_streams=1, **aws)
    got, _ = _run(batch, 7, num_streams=4, sub_batch=1, **aws)
    assert len({want[i].tobytes() for i in range(4)}) == 4   # (the pairs differ: a wrong offset would show)
    np.testing.assert_array_equal(got, want)


def test_profiling_across_lanes():
    """CBCA + 4-path SGM with profiling on: four one-pair groups over three streams report the kernel names of a
    one-group, one-stream run, each with four times its launches (a bracket is one record whatever the pairs)."""
    batch = S.make_batch(4, 30, 52, 32, first_index=910)
    cbca = dict(aggregation="CBCA", optimization=1, sgm_paths=4)
    want, one = _run(batch, 31, profile=True, num_streams=1, sub_batch=0, **cbca)
    got, four = _run(batch, 31, profile=True, num_streams=3, sub_batch=1, **cbca)
    assert one and all(v["launches"] > 0 for v in one.values())
    assert sorted(four) == sorted(one)
    assert {k: v["launches"] for k, v in four.items()} == {k: 4 * v["launches"] for k, v in one.items()}
    np.testing.assert_array_equal(got, want)


NL = dict(aggregation="NL", optimization=1, num_streams=1)
NL_SHAPE = (2, 24, 36, 16)   # pairs, rows, cols, D


@functools.lru_cache(maxsize=None)
def _nl_sets():
    """Two image sets and, for each, a fresh context's maps."""
    n, H, W, D = NL_SHAPE
    sets = [S.make_batch(n, H, W, D, first_index=i) for i in (920, 930)]
    fresh = [_run(b, D - 1, **NL)[0] for b in sets]
    for f in fresh:
        f.setflags(write=False)
    assert not np.array_equal(fresh[0], fresh[1])
    return sets, fresh


def test_nl_pipelined_front_alternating_sets():
    """NL + SGM on one view and one stream: sm_run's prep, cost volume and trees run on the front stream into the
    call's record / table set and cost-volume set.  Three calls on one context, the images alternating, use both
    sets (0, 1, 0); then the reference-ordered entry points take the path through run_nl without that front."""
    n, H, W, D = NL_SHAPE
    sets, fresh = _nl_sets()
    sb = StereoBatch(D - 1, H, W, n, device=0, **NL)
    try:
        for call, which in enumerate((0, 1, 0)):
            sb.upload(*(sets[which][k] for k in KEYS))
            np.testing.assert_array_equal(sb.run(0.3), fresh[which], err_msg=f"call {call}")
        lib, ctx = sb._lib, sb._ctx
        _capi.check(lib, ctx, lib.sm_cost_calculate(ctx), "sm_cost_calculate")
        _capi.check(lib, ctx, lib.sm_solve_all(ctx, 1, 0.3), "sm_solve_all")
        _capi.check(lib, ctx, lib.sm_disp_optimize(ctx, None), "sm_disp_optimize")
        np.testing.assert_array_equal(sb.download(), fresh[0], err_msg="reference-ordered calls")
    finally:
        sb.close()
