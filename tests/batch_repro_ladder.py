"""The entry ladder of the bit-reproducible batch (include/spllt_hip_batch_repro.h), shared by
tests/test_batch_repro_cpu.py and tests/test_batch_repro_gpu.py.  The family is not in the recorded table of
tests/capi_ladder.py (its header says why); as in batch_solve_many_ladder.py every entry point is called in every
handle state with every argument variant, and the return code has to be the one RECORDED for the same variant of its
sibling in tests/golden/capi_ladder_{cpu,gpu}.json:

    spllt_hip_solve_repro_batch        spllt_hip_solve_batch
    spllt_hip_solve_repro_batch_dev    spllt_hip_solve_batch_dev
    spllt_hip_set_batch_reproducible   spllt_hip_set_reproducible_solve (a plain setter that returns the previous
                                       setting and refuses "on" on a partitioned handle)
    spllt_hip_batch_repro_info         spllt_hip_solve_sparse_info (a plain reader of int64 counters)
    spllt_hip_release_batch_repro      spllt_hip_release_batch

The walk itself is batch_solve_many_ladder.check_state, run on this family's tables."""
import batch_solve_many_ladder as base

ENTRIES = {
    "spllt_hip_solve_repro_batch": (lambda c: [2, base._H(c), c.n, 0], base._job, "spllt_hip_solve_batch"),
    "spllt_hip_solve_repro_batch_dev": (lambda c: [2, c.D(), c.n, 0, 0], base._job, "spllt_hip_solve_batch_dev"),
    "spllt_hip_set_batch_reproducible": (lambda c: [0], {"on": {0: 1}}, "spllt_hip_set_reproducible_solve"),
    "spllt_hip_batch_repro_info": (lambda c: [base._I64(c)], {"null": {0: None}}, "spllt_hip_solve_sparse_info"),
}
RELEASE = ("spllt_hip_release_batch_repro", "spllt_hip_release_batch")
ROWS = 2 * 6 + 2 + 2 + 2      # per handle state

golden = base.golden


def check_state(c, state, table):
    """base.check_state with this family's entry points; returns the number of rows checked"""
    saved = base.ENTRIES, base.RELEASE
    base.ENTRIES, base.RELEASE = ENTRIES, RELEASE
    try:
        return base.check_state(c, state, table)
    finally:
        base.ENTRIES, base.RELEASE = saved
