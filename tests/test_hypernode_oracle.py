"""``reference.hypernode_mask`` (the rule mode 3 of ``vamd_domain_mask``
reproduces) on hand-written trees, and the two scheduler scenarios the
host-side domain choice gets wrong, through ``run_plan_torch``."""

import numpy as np
import pytest
import torch

import _hypernode_cases as hc
from volcano_amd.ops import reference as ref

# 12 nodes, 4 leaves; racks 0..3, pods (0,1) (2,3), one spine.  Node 11 is
# in no hypernode.
LEAF_OF = [0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, -1]
RACKS = [(0, 1), (1, 2), (2, 3), (3, 4)]
PODS = [(0, 2), (2, 4)]
SPINE = [(0, 4)]
#                      rack0     rack1     rack2  rack3     none
CAP = [2, 1, 1, 2, 2, 2, 3, 0, 1, 1, 2, 5]      # C = 4, 6, 3, 4

CASES = {
    # name: (tiers, need, pin, soft, cap) -> kept leaf range or None/"all"
    "lowest-tier-wins": ([[(1, 2)], [(0, 1)]], 4, None, False, CAP, (1, 2)),
    "tightest-fit": ([RACKS], 3, None, False, CAP, (2, 3)),
    "equal-C-lower-index": ([RACKS], 4, None, False, CAP, (0, 1)),
    "pin-inside": ([RACKS, PODS], 1, (3, 4), False, CAP, (3, 4)),
    "pin-straddles": ([RACKS, PODS], 1, (0, 2), False, CAP, (0, 2)),
    "need-above-leaf": ([RACKS, PODS], 7, None, False, CAP, (2, 4)),
    "need-above-all-hard": ([RACKS, PODS, SPINE], 18, None, False, CAP, None),
    "need-above-all-soft": ([RACKS, PODS, SPINE], 18, None, True, CAP, "all"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_rule_on_a_small_tree(name):
    tiers, need, pin, soft, cap, want = CASES[name]
    cap = torch.tensor(cap, dtype=torch.int32)
    score = torch.arange(12, dtype=torch.float32)
    score[cap == 0] = ref.NEG_INF
    before = (score.clone(), cap.clone())
    leaf_of = torch.tensor(LEAF_OF, dtype=torch.int32)
    table = torch.from_numpy(ref.hypernode_table(tiers, need, 4, pin, soft))
    ref.hypernode_mask(score, cap, leaf_of, table, 4)
    if want == "all":
        keep = torch.ones(12, dtype=torch.bool)
    elif want is None:
        keep = torch.zeros(12, dtype=torch.bool)
    else:
        keep = (leaf_of >= want[0]) & (leaf_of < want[1])
        assert not keep[11]              # leaf_of = -1 is always masked
    assert torch.equal(score[keep], before[0][keep])
    assert torch.equal(cap[keep], before[1][keep])
    assert (score[~keep] == ref.NEG_INF).all() and (cap[~keep] == 0).all()


def test_leaf_sums_do_not_wrap():
    score, cap, leaf_of, table = hc.huge_case()
    assert int(np.sum(cap[:2], dtype=np.int32)) < 11     # what int32 gives
    score, cap = torch.from_numpy(score), torch.from_numpy(cap)
    ref.hypernode_mask(score, cap, torch.from_numpy(leaf_of),
                       torch.from_numpy(table), 2)
    assert cap.tolist() == [hc.INT_MAX, hc.INT_MAX, 0, 0, 0]
    assert score.tolist()[:2] == [1, 2] and (score[2:] == ref.NEG_INF).all()


def test_table_checks():
    good = ref.hypernode_table([RACKS, PODS], 2, 4)
    ref.check_hypernode_table(good, 4)
    for at, value in ((0, 0), (1, 0), (5, 9), (7, 99), (-1, 5)):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(ValueError):
            ref.check_hypernode_table(bad, 4)


def test_two_gangs_in_one_cycle_take_different_racks():
    binds = hc.schedule("two-gangs")
    assert len(binds) == 8
    r1, r2 = hc.racks_of(binds, "g1"), hc.racks_of(binds, "g2")
    assert len(r1) == 1 and len(r2) == 1 and r1 != r2


def test_fragmented_rack_is_passed_over():
    binds = hc.schedule("fragmented")
    assert len(binds) == 2 and hc.racks_of(binds, "g1") == {"b"}


def test_without_exact_the_host_choice_stays():
    """The switch is off by default: the same cycle plans no hypernode
    class and reaches the parent's (worse) result."""
    assert hc.racks_of(hc.schedule("fragmented", exact=False), "g1") == set()
