"""A small randomised soak of LambdaMART's leaf regularisation ("Leaf regularisation"): 20 seeded requests
over the three keys composed with the other keys the refusals allow, 6 trees each, every stage held to the restatement bit
for bit (tests/lambdamart_reg_stages.py)."""
import numpy as np
import pytest

from tests import lambdamart_composed_model as cmod
from tests import lambdamart_reg_stages as rs

pytestmark = pytest.mark.gpu


def soak_case(i):
    """Case i: the small shape under a seed of its own, the three keys and the other keys drawn from a generator of its own."""
    rng = np.random.default_rng([20250317, i])
    X, y, qid = rs.small_dataset(int(rng.integers(1, 10 ** 6)))
    names = cmod._names(qid)
    p = dict(num_trees=6, seed=int(rng.integers(0, 2 ** 63)), max_depth=int(rng.integers(2, 7)), min_leaf_support=int(rng.integers(1, 12)),
             split_candidates=int(rng.choice([2, 5, 16, 64, 65, 256])), learning_rate=float(rng.choice([0.1, 0.5])),
             lambda_l2=float(rng.choice([0.0, 2.0 ** -6, 1.0])),
             lambda_l1=float(rng.choice([0.0, 2.0 ** -10, 2.0 ** -6, 2.0 ** -3])), max_delta_step=float(rng.choice([0.0, 0.25, 2.0, 1e300])),
             path_smooth=float(rng.choice([0.0, 0.5, 8.0, 100.0])))
    if p["lambda_l1"] == p["max_delta_step"] == p["path_smooth"] == 0.0:
        p["path_smooth"] = 4.0
    shape = rng.random()
    if shape < 0.35:
        p["max_leaves"], p["max_depth"] = int(rng.integers(2, 12)), int(rng.integers(3, 10))
    elif shape < 0.55:
        p["symmetric_trees"], p["path_smooth"] = True, 0.0
        if p["lambda_l1"] == p["max_delta_step"] == 0.0:
            p["max_delta_step"] = 0.5
    if not p.get("symmetric_trees") and rng.random() < 0.4:
        p["monotone_constraints"] = {str(int(rng.integers(0, 5))): int(rng.choice([-1, 1]))}
    if not p.get("symmetric_trees") and rng.random() < 0.4:
        a = float(rng.choice([0.1, 0.3, 0.5]))
        p["goss_top_rate"], p["goss_other_rate"] = a, float(rng.choice([0.1, 0.25, 0.5]))
    if rng.random() < 0.4:
        p["query_sampling_rate"] = float(rng.choice([0.4, 0.8]))
    if rng.random() < 0.4:
        p["feature_sampling_rate"] = float(rng.choice([0.4, 0.8]))
    if rng.random() < 0.3:
        p["validation_queries"] = names[int(rng.integers(0, 3))::4]
    p["objective"] = str(rng.choice(["ndcg", "ndcg", "map", "mrr", "xendcg"]))
    if p["objective"] != "xendcg" and rng.random() < 0.4:
        p["truncation_level"] = int(rng.integers(1, 6))
    if rng.random() < 0.3:
        p.update(drop_rate=0.5, skip_drop=0.0)
    return X, y, qid, names, p


@pytest.mark.parametrize("i", range(20))
def test_soak(i):
    X, y, qid, names, p = soak_case(i)
    g, c = rs.datasets(X, y, qid)
    try:
        rs.stagewise(g, c, X, y, "ndcg@5", p, names=names)
    except AssertionError as e:
        raise AssertionError("case %d: %r\n%s" % (i, p, e)) from e
