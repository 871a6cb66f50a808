"""Host-side arithmetic of the order selection (no GPU, no library call): how ``MultiOrderModel`` combines walk counts into degrees of freedom
and likelihood terms into log-likelihoods, fed with hand-computed terms of the reference's toy examples and checked against its known answers
(reference tests/core/test_multi_order_model.py:45-162)."""
import numpy as np

from pathpyg_amd.core.multi_order_model import dof_from_walk_counts, llh_from_terms

LOG = np.log


def test_dof_from_walk_counts():
    # walks a-c-d and b-c-e: topology a->c, b->c, c->d, c->e on 5 nodes.  Walks of length 1: the 4 edges, started by a, b, c; of length 2:
    # a-c-d, a-c-e, b-c-d, b-c-e, started by a and b
    totals, starts = [4, 4], [3, 2]
    assert [dof_from_walk_counts(5, totals, starts, k) for k in (0, 1, 2)] == [4, 5, 7]
    # a line a-b-c-d: 3, 2, 1, 0 walks of length 1..4, started by as many nodes: every order adds nothing
    assert [dof_from_walk_counts(4, [3, 2, 1, 0], [3, 2, 1, 0], k) for k in range(5)] == [3] * 5
    # counts beyond int64 and float64's integers stay exact: the complete digraph with loops on 216 nodes
    n = 216
    totals, starts = [n ** (k + 1) for k in range(1, 10)], [n] * 9
    want = n - 1 + sum(n ** (k + 1) - n for k in range(1, 10))
    got = dof_from_walk_counts(n, totals, starts, 9)
    assert type(got) is int and got == want and got > 2 ** 63
    assert dof_from_walk_counts(n, totals, starts, 3) == n - 1 + sum(n ** (k + 1) - n for k in (1, 2, 3))


def test_llh_from_terms_toys():
    # (1) walks a-c-d, b-c-e, weight 1.  Z: both start nodes hold 1 of 6 positions.  T1: a->c and b->c are certain, c->d and c->e 1/2 each.
    # I1: the rows of the first transitions (a, b) have one successor.  T2: (a,c)->(c,d) and (b,c)->(c,e) are certain.
    z, t1, i1, t2 = 2 * LOG(1 / 6), 2 * 1 * LOG(1 / 2), 0.0, 0.0
    assert np.isclose(llh_from_terms(z, [], t1), LOG(1 / 6) * 2 + 0 + 2 * LOG(1 / 2))
    assert np.isclose(llh_from_terms(z, [i1], t2), LOG(1 / 6) * 2 + 0 + 0)
    # (2) a-c-d, b-c-e, a-c-e, b-c-d: 4 walks start at nodes with 2 of 12 positions; c->d, c->e weigh 2 of 4; at order 2 every (x,c) splits 1 : 1
    z, t1, i1, t2 = 4 * LOG(2 / 12), 2 * 2 * LOG(2 / 4), 0.0, 4 * 1 * LOG(1 / 2)
    assert np.isclose(llh_from_terms(z, [], t1), LOG(2 / 12) * 4 + 0 + 4 * LOG(1 / 2))
    assert np.isclose(llh_from_terms(z, [i1], t2), LOG(1 / 6) * 4 + 0 + 4 * LOG(1 / 2))
    # (3) a, a-b, a-b-c: three walks start at a (3 of 6 positions); every transition is certain
    z = 3 * LOG(3 / 6)
    assert np.isclose(llh_from_terms(z, [], 0.0), LOG(3 / 6) * 3)
    assert np.isclose(llh_from_terms(z, [0.0], 0.0), LOG(3 / 6) * 3)


def test_llh_from_terms_adds_left_to_right():
    # (1e16 + 1.0) + 1.0 loses both ones in float64; any other association keeps at least one
    assert llh_from_terms(1e16, [1.0], 1.0) == 1e16
    assert llh_from_terms(1.0, [1.0], 1e16) == 1e16 + 2.0
    assert llh_from_terms(-3.5, [], 0.25) == -3.25
