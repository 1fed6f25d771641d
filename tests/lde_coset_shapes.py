"""The LDE shapes of tests/test_gpu_lde_cosets.py whose point is a launch property the GPU cannot show: how many columns a workgroup
of the strided and local passes loops over (csrc/ntt_plan.h: pick_cols_per_block) and how ntt_front10 splits its cosets into
launches (front10_launch_cosets, front10_cols_per_block).  tests/ntt_plan_check.cpp holds the same rows as literals, computes each
through the header and prints them; tests/test_ntt_plan_host.py compares its lines with the ones below, so a change of the 4096
threshold or of the eight cosets per launch fails on the host instead of turning the GPU cases back into one column per workgroup."""

# More than one column per workgroup.  cpb is what every strided and local pass of the plan gets (they share tiles, columns and
# cosets); groups = ceil(n_cols / cpb) workgroups per tile and coset, the last of them with `last` columns.
MULTI_COLUMN = [
    dict(log_n=12, aligned=1, n_cols=127, n_cosets=64, plan="L12", cpb=2, groups=64, last=1),
    dict(log_n=18, aligned=1, n_cols=3, n_cosets=64, plan="F4 S4 L10", cpb=8, groups=1, last=3),
    dict(log_n=18, aligned=0, n_cols=3, n_cosets=64, plan="F5 S4 L9", cpb=8, groups=1, last=3),
    dict(log_n=17, aligned=1, n_cols=3, n_cosets=64, plan="R1 S4 L12", cpb=2, groups=2, last=1),
]

# The two-pass plan at 2^22, one column: launches = (first coset, cosets, columns per workgroup) of every ntt_front10 launch.
FRONT10 = [
    dict(tiled=0, n_cols=1, log_lde=2, begin=1, count=3, launches=[(0, 3, 1)]),
    dict(tiled=0, n_cols=1, log_lde=4, begin=3, count=9, launches=[(0, 8, 1), (8, 1, 1)]),
    dict(tiled=1, n_cols=1, log_lde=4, begin=5, count=11, launches=[(0, 8, 8), (8, 3, 1)]),
]


def multi_column_line(c):
    return 'cpb log_n=%d aligned=%d n_cols=%d n_cosets=%d plan="%s" cpb=%d groups=%d last=%d' % (
        c["log_n"], c["aligned"], c["n_cols"], c["n_cosets"], c["plan"], c["cpb"], c["groups"], c["last"])


def front10_line(c):
    return "front10 tiled=%d n_cols=%d n_cosets=%d launches=%s" % (
        c["tiled"], c["n_cols"], c["count"], ",".join("%d:%d:%d" % l for l in c["launches"]))
