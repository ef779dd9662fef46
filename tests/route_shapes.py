"""Which fetch stage a search call runs, restated in Python from csrc/rq_plan.h: nb_default, the exact rule 2 * nb >= nbins and the
greedy cut of a batch into passes of 256 / 128 / 64 queries.  tests/test_route_shapes.py pins every line of this file to plan_call
itself (tests/native/plan_check.cpp, on the host), so a GPU test may say "this call is planned as the approximate scan in these
passes" and compare the counters of the index with it.  All of it holds for an index at its default options ("wide_batch" = 1,
"wide256_8" on, "fast_tail" on, "slack_bins" = -1) whose fp16 scan is usable (no shard of fp16-subnormal rows).

The shapes at which the routes built on the plain search -- MMR, grouped, group members, per-query filters -- are pinned on the
approximate scan (tests/test_gpu_routes_scanned.py) are listed here too, so that the host check covers exactly what the GPU runs."""
from collections import namedtuple

FAST_MAX_K = 320                   # RQ_FAST_MAX_K: the fast tail's largest k
BIN_ROWS = 64
CU_COUNT = 256                     # compute units of an MI355X (and of a default rq_index on the host)

Plan = namedtuple("Plan", "exact fast npass pass_q nb")
Shape = namedtuple("Shape", "rows dim row_pad scan8")


def nbins(rows):
    return (rows + BIN_ROWS - 1) // BIN_ROWS


def nb_default(m):
    """Bins re-scored per query of a search for m rows."""
    return m + max(8, m // 8)


def is_exact(rows, m):
    """Fewer than two bins per wanted bin: every bin is re-scored in fp64 and no corpus scan runs."""
    return 2 * nb_default(m) >= nbins(rows)


def passes(B, narrow=False, image=False):
    """Queries per corpus pass, widest first: 256 while more than 128 queries remain, then 128, then 64.  Rows of 384 elements
    (narrow): 128 then 64.  The int8 image, for calls of more than 64 queries: 256, 128, 64."""
    out, left = [], B
    while left > 0:
        if narrow:
            qb = 128 if left > 64 else 64
        else:                                  # (image: the same cut while "wide256_8" is on, in kernels of its own)
            qb = 256 if left > 128 else (128 if left > 64 else 64)
        out.append(qb)
        left -= qb
    return out


def wide_grid(rows):
    """Workgroups of a pass that runs ONE per CU: as many partition maxima as the fast tail's threshold can choose from."""
    return min(nbins(rows), CU_COUNT)


def plan(rows, B, m, narrow=False, image=False):
    """The plan of a search of B queries for m rows at the default nb: (exact, fast, npass, pass_q, nb).  The fast tail serves up to
    FAST_MAX_K rows -- but no more than a wide pass over the fp16 rows (any of more than 64 queries on rows of 768 elements; a
    call's first pass is its widest) has workgroups (rq_plan.h fast_tail_fits); the int8 image is left to its own ladder."""
    exact = is_exact(rows, m)
    cut = passes(B, narrow, image)
    wide = not narrow and not image and cut[0] > 64
    fast = (not exact) and m <= FAST_MAX_K and not (wide and min(m, rows) > wide_grid(rows))
    return Plan(exact, fast, len(cut), tuple(cut), nbins(rows) if exact else nb_default(m))


# ---- the shapes of tests/test_gpu_routes_scanned.py ----------------------------------------------------------------------------
SHAPES = {
    "S1": Shape(12_805, 768, 768, 0),      # 201 bins, a ragged last bin: approximate for every fetch of m <= 80 (nb = 90, 180 < 201)
    "S2": Shape(49_157, 768, 768, 0),      # 769 bins: approximate up to m = 330 (nb = 371, 742 < 769)
    "S1n": Shape(12_805, 384, 384, 0),     # the narrow layout: passes of 128 then 64
    "S1i": Shape(12_805, 768, 768, 2),     # "scan8" = 2: the int8 image is the operand of every unfiltered fetch
}
# (shape, B, m) of every fetch the GPU tests expect on the approximate scan; m = 80 is a grouped search at k = 10 and the default
# "group_fetch" of 8, m = 32 one at k = 4; B <= 15 are the groups of the per-query filter calls (21 filters dealt to 130 / 300 queries)
FETCHES = (
    [("S1", B, m) for B in (16, 130, 300) for m in (10, 64)] + [("S1", B, m) for B in (3, 130, 300) for m in (32, 80)] +
    [("S1", B, 10) for B in (6, 7, 14, 15)] +
    [("S2", 130, m) for m in (257, 320, 330)] +
    [("S1n", 200, m) for m in (32, 80)] +
    [("S1i", B, m) for B in (130, 300) for m in (64, 80)] + [("S1i", 300, 10)]
)


def image_wanted(rows, m):
    """scan8_wanted at "scan8" = 2 on rows of 768 elements: an approximate call within the fast tail's range."""
    return m <= FAST_MAX_K and not is_exact(rows, m)


def uses_image(name, B, m, filtered=False):
    """A filtered fetch never reads the int8 image, nor do rows of 384 elements."""
    sh = SHAPES[name]
    return sh.scan8 == 2 and sh.row_pad != 384 and not filtered and image_wanted(sh.rows, m)


def shape_plan(name, B, m, filtered=False):
    """The plan of one fetch on a named shape."""
    sh = SHAPES[name]
    return plan(sh.rows, B, m, narrow=sh.row_pad == 384, image=uses_image(name, B, m, filtered))
