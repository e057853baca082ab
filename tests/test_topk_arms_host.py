"""The top-k arm table (tests/topk_arms.py) against its own predictor: every case reaches the arm it is named for.  No GPU."""
import pytest

import topk_arms


@pytest.mark.parametrize("name", sorted(topk_arms.CASES))
def test_case_reaches_its_arm(name):
    _, n, k, expect = topk_arms.CASES[name]
    rows = topk_arms.rows(name)
    assert rows.shape[1] == n
    for r, row in enumerate(rows):
        got = topk_arms.predict(row, k)
        for field, want in expect.items():
            assert want(got[field]) if callable(want) else got[field] == want, (name, r, field, got)
