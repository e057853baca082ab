"""CPU: the numpy restatement of the grouping (tests/cluster_ref.py::dbscan_ref), which test_gpu_cluster.py holds the device against,
equals scikit-learn's DBSCAN on the 0/1 matrix of the relation -- the oracle pinned to an implementation by somebody else.  The
relation comes from float64 numpy under the margin condition; no device and nothing of the package is involved."""
import numpy as np
import pytest

import cluster_ref as cr

sklearn_cluster = pytest.importorskip("sklearn.cluster")


def _sklearn_labels(rel, m):
    dist = 1.0 - rel.astype(np.float64)                        # neighbours at distance 0, everything else at 1
    return sklearn_cluster.DBSCAN(eps=0.5, min_samples=m, metric="precomputed").fit(dist).labels_.astype(np.int32)


@pytest.fixture(scope="module")
def relations():
    return {g: cr.relation64(cr.unit_rows(cr.chain_fixture(g)), cr.T) for g in cr.FIXTURE_GROUPS}


@pytest.mark.parametrize("groups", cr.FIXTURE_GROUPS)
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_restatement_equals_sklearn_on_the_fixtures(relations, groups, m):
    rel = relations[groups]
    assert len(rel) == cr.FIXTURE_ROWS[groups]
    got = cr.dbscan_ref(rel, m)
    np.testing.assert_array_equal(got, _sklearn_labels(rel, m))
    if m == 5:
        assert (got == -1).all()
    if m == 1:
        assert (got >= 0).all()


def test_fixture_545_has_cores_borders_and_noise():
    rel = cr.relation64(cr.unit_rows(cr.chain_fixture(90)), cr.T)
    labels, core = cr.dbscan_ref(rel, 3), cr.core_rows(rel, 3)
    assert (int(labels.max()) + 1, int(core.sum()), int(((labels >= 0) & ~core).sum()), int((labels < 0).sum())) == (80, 360, 160, 25)


@pytest.mark.parametrize("order", cr.CONTESTED_ORDERS)
def test_contested_border_takes_the_smaller_label(order):
    rel = cr.relation64(cr.unit_rows(cr.plane_rows(cr.CONTESTED_ANGLES[order])), cr.T)
    contested = order.index(0)
    core = cr.core_rows(rel, 4)
    assert not core[contested] and len(set(cr.dbscan_ref(rel, 4)[rel[contested] & core])) == 2      # a core neighbour in each cluster
    got = cr.dbscan_ref(rel, 4)
    assert got.tolist() == cr.CONTESTED_LABELS
    np.testing.assert_array_equal(got, _sklearn_labels(rel, 4))
