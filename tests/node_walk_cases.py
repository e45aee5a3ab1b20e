"""The small grids and lowered plan limits under which the node walk of hj_index_dev.h takes its head paths: shared by
tests/test_node_index_host.py (the plan and the decode, every node, no device) and tests/test_gpu_node_walk.py (the kernels).

A FORM is a pair of limits (HJ_INDEX_TAIL_BELOW, HJ_INDEX_LAUNCH_BLOCKS; None: unset) and what the published plan must then say:
  head      every axis but the last is a head axis and the tail is shorter than a wave: whole waves return early, every head
            axis is reached by the carry;
  middle    a split in the middle with more than one workgroup per head index, the last one partly filled: split_block's
            quotient path.  Only a grid with a proper suffix of more than 256 nodes has it;
  launches  `head` over three launches or more, the last one shorter, and (where the grid has two head axes) a launch whose first
            head index is non-zero on two of them: the per-launch h0 and node0;
  middle-launches   both at once.
"""
import numpy as np

ENV_TAIL, ENV_BLOCKS = "HJ_INDEX_TAIL_BELOW", "HJ_INDEX_LAUNCH_BLOCKS"
WAVE, BLOCK = 64, 256

# grid -> head indices per launch of the `launches` form (all of them leave a shorter last launch)
GRIDS = {(19, 17): 7, (9, 8, 7): 13, (6, 5, 4, 5): 23, (5, 3, 4, 3, 3): 41, (6, 5, 7, 5, 6, 8): 1000, (5, 3, 3, 2, 3, 3): 61,
         (3, 1, 4, 1, 5, 1): 13}
# grid -> (the tail's first axis, head indices per launch) of the `middle` forms
MIDDLE = {(6, 5, 7, 5, 6, 8): (2, 7)}
ONE_NODE_AXES = (3, 1, 4, 1, 5, 1)           # not a grid of the measure library: an axis has at least two nodes there


def nodes_of(N):
    total = 1
    for n in N:
        total *= int(n)
    return total


def forms_of(N):
    return ["head", "launches"] + (["middle", "middle-launches"] if N in MIDDLE else [])


def limits(N, form):
    """(HJ_INDEX_TAIL_BELOW, HJ_INDEX_LAUNCH_BLOCKS) of a form on grid N, None for a limit left unset."""
    if form == "head":
        return 1, None                       # at or below N[last]: counts as just above it
    if form == "launches":
        return 1, GRIDS[N]                   # one workgroup per head index
    ft, per_launch = MIDDLE[N]
    tail = nodes_of(N[ft:])
    chunks = -(-tail // BLOCK)
    return tail + 1, (None if form == "middle" else per_launch * chunks + chunks - 1)      # not a multiple of chunks: rounded down


def set_limits(monkeypatch, N=None, form=None):
    """The form's limits into the environment; no form: both unset."""
    for name, v in zip((ENV_TAIL, ENV_BLOCKS), limits(N, form) if form else (None, None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def first_heads(p, N):
    """The multi-index over the head axes of every launch's first head index."""
    return [tuple(int(v) for v in np.unravel_index(l * p.heads_per_launch, N[:p.first_tail])) for l in range(p.launches)]


def check_form(p, N, form):
    """The published plan `p` of grid N says what the form means to run."""
    nd, total = len(N), nodes_of(N)
    assert p.total == total and p.head * p.tail == total and p.tail == nodes_of(N[p.first_tail:])
    assert (p.chunks - 1) * BLOCK < p.tail <= p.chunks * BLOCK
    assert (p.launches - 1) * p.heads_per_launch < p.head <= p.launches * p.heads_per_launch
    assert p.blocks_last == (p.head - (p.launches - 1) * p.heads_per_launch) * p.chunks
    assert p.launches == 1 or p.blocks_full == p.heads_per_launch * p.chunks
    if form in ("head", "launches"):
        assert p.first_tail == nd - 1 and p.tail == N[-1] < WAVE and p.chunks == 1 and p.head > 1
    else:
        assert 0 < p.first_tail == MIDDLE[N][0] < nd - 1 and p.tail > BLOCK and p.tail % BLOCK != 0 and p.chunks > 1 and p.head > 1
    if form in ("head", "middle"):
        assert p.launches == 1 and p.heads_per_launch == p.head
    else:
        assert p.launches >= 3 and p.head % p.heads_per_launch != 0 and p.blocks_last < p.blocks_full
        if p.first_tail >= 2:
            assert any(sum(1 for v in h if v) >= 2 for h in first_heads(p, N)), first_heads(p, N)
    return p
