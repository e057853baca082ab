"""Shared by test_gpu_cluster.py and test_cluster_reference.py: the fixtures of the clustering tests and a pure-numpy restatement of
the grouping CharacterFeatureIndex.cluster computes.  Nothing here imports the package.

Relation     j in N(i)  <=>  1 - s(i, j) < T, for every j (j == i included).
Grouping     DBSCAN in its canonical, order-independent form:
               core     |N(i)| >= min_samples
               cluster  connected components of the core rows under the relation, numbered 0, 1, ... by smallest core row
               border   a non-core row with core neighbours takes the SMALLEST label among them
               noise    everything else, -1
"""
import numpy as np

T = 0.1                      # 1 - cos 0.30 = 0.0447 < T < 0.175 = 1 - cos 0.60
STEP = 0.30
MARGIN = 1e-3                # no float64 difference may lie this close to T: 20 x the float32 chain's worst-case error at K = 768 (4.6e-5)
FIXTURE_GROUPS = (6, 40, 90)                     # -> 41, 244, 545 rows
FIXTURE_ROWS = {6: 41, 40: 244, 90: 545}
CONTESTED_ANGLES = np.array([0.0, .3, .55, .6, .65, -.3, -.55, -.6, -.65])
CONTESTED_ORDERS = ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 0, 4, 3, 2, 1], [1, 2, 3, 4, 0, 5, 6, 7, 8])
CONTESTED_LABELS = [0, 0, 0, 0, 0, 1, 1, 1, 1]


def orthonormal(dim, seed):
    """rows: an orthonormal basis of R^dim (QR of a seeded normal matrix), float64"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((dim, dim)))
    return q.T


def chain_fixture(groups, dim=768, seed=20260119):
    """Group g is a chain of L_g = 2 + (7 g mod 9) rows at 0.30 rad steps in the plane (Q[2g], Q[2g + 1]); five isolated rows
    Q[-1] .. Q[-5]; shuffled; every row scaled by a factor in [0.5, 3].  float32 [N, dim]."""
    assert dim >= 2 * groups + 5
    Q = orthonormal(dim, seed)
    rows = []
    for g in range(groups):
        for t in range(2 + (7 * g) % 9):
            rows.append(np.cos(STEP * t) * Q[2 * g] + np.sin(STEP * t) * Q[2 * g + 1])
    rows.extend(Q[-k] for k in range(1, 6))
    rows = np.stack(rows)
    rng = np.random.default_rng(seed + 1)
    rows = rows[rng.permutation(len(rows))]
    rows = rows * rng.uniform(0.5, 3.0, (len(rows), 1))
    assert len(rows) == FIXTURE_ROWS.get(groups, len(rows))
    return rows.astype(np.float32)


def plane_rows(angles, dim=768, seed=7):
    Q = orthonormal(dim, seed)
    a = np.asarray(angles, dtype=np.float64)[:, None]
    return (np.cos(a) * Q[0] + np.sin(a) * Q[1]).astype(np.float32)


def unit_rows(feats):
    """what CharacterFeatureIndex.add_features stores: float32 rows divided by their float32 norm (all-zero rows stay)"""
    feats = np.asarray(feats, dtype=np.float32)
    n = np.sqrt((feats ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return np.where(n > 0, feats / np.where(n > 0, n, 1), feats).astype(np.float32)


def differences64(unit):
    u = np.asarray(unit, dtype=np.float64)
    return 1.0 - u @ u.T


def relation64(unit, threshold, margin=MARGIN):
    """The relation from float64 numpy, trusted only under the margin condition, which is asserted here: bool [n, n]."""
    d = differences64(unit)
    t = float(np.float32(threshold))
    gap = float(np.min(np.abs(d - t)))
    assert gap >= margin, "a difference lies %.3g from the threshold, the margin condition asks for %.3g" % (gap, margin)
    return d < t


def lists_of(rel):
    """(ptr int64 [n + 1], ids int32) of a bool relation matrix, ids ascending per row"""
    ptr = np.zeros(len(rel) + 1, dtype=np.int64)
    np.cumsum(rel.sum(axis=1), out=ptr[1:])
    return ptr, np.nonzero(rel)[1].astype(np.int32)


def dbscan_ref(rel, min_samples):
    """labels int32 [n] by the definition at the top, from the bool relation matrix"""
    rel = np.asarray(rel, dtype=bool)
    n = len(rel)
    core = rel.sum(axis=1) >= min_samples
    labels = np.full(n, -1, dtype=np.int32)
    clusters = 0
    for i in range(n):                               # ascending: a cluster is met first at its smallest core row
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = clusters
        stack = [i]
        while stack:
            for j in np.flatnonzero(rel[stack.pop()] & core & (labels < 0)):
                labels[j] = clusters
                stack.append(int(j))
        clusters += 1
    for i in np.flatnonzero(~core):
        near = labels[rel[i] & core]
        if len(near):
            labels[i] = near.min()
    return labels


def core_rows(rel, min_samples):
    return np.asarray(rel, dtype=bool).sum(axis=1) >= min_samples


def relabel_by_smallest_core(labels, core):
    """the same membership, clusters renumbered by their smallest core row"""
    labels = np.asarray(labels)
    first = {}
    for i in np.flatnonzero(core):
        first.setdefault(int(labels[i]), int(i))
    order = {c: k for k, c in enumerate(sorted(first, key=first.get))}
    return np.array([order[int(c)] if c >= 0 else -1 for c in labels], dtype=np.int32)
